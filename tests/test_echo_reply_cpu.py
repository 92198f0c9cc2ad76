"""CPU-side checks of verify_echo_reply (smol_csum_batch_verify_echo_reply): the symbol, the cfg and entry
structs in their three spellings (C, ctypes, numpy), the argument errors, and tests/echo_ref.py on the
reference's own known-answer echo packet.  No kernel is launched here."""
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
from tests import echo_ref as R
from tests import pktgen as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "smol_csum_batch_verify_echo_reply"

# src/wire/icmpv4.rs:640-671: ECHO_PACKET_BYTES and ECHO_DATA_BYTES (tests/golden/kat.json carries the packet
# as "icmpv4_echo"; restated here for a tree without it)
ECHO_PACKET_BYTES = bytes([0x08, 0x00, 0x8E, 0xFE, 0x12, 0x34, 0xAB, 0xCD, 0xAA, 0x00, 0x00, 0xFF])
ECHO_DATA_BYTES = bytes([0xAA, 0x00, 0x00, 0xFF])


def test_symbol_declared_exported_and_listed():
    with open(os.path.join(ROOT, "include", "smolcsum.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    L = smoltcp_amd.lib()
    assert re.search(r"\b%s\s*\(" % NAME, text)
    assert hasattr(L, NAME) and NAME in _lib.ABI_SYMBOLS
    assert "smol_csum_echo_cfg_t" in text and "smol_csum_echo_t" in text
    for flag, val in (("REQUEST", 1), ("ANSWERED", 2), ("WRITTEN", 4), ("SEND", 8), ("HOST", 16)):
        m = re.search(r"#define\s+SMOL_ECHO_%s\s+0x([0-9a-fA-F]+)u" % flag, text)
        assert m and int(m.group(1), 16) == val == getattr(E, "ECHO_" + flag) == getattr(R, flag)
    assert L.smol_csum_abi_version() == 6  # additive: the version stays


_C_PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include "smolcsum.h"
int main(void) {
    smol_csum_echo_cfg_t c;
    smol_csum_echo_t e;
    memset(&c, 0, sizeof c);
    memset(&e, 0, sizeof e);
    for (int i = 0; i < 4; ++i) c.bcast_v4[i] = (uint8_t)(1 + i), c.reserved[i] = (uint8_t)(5 + i);
    e.frame_len = 0x04030201u, e.data_off = 0x0605, e.head_len = 7, e.flags = 8;
    printf("{\"cfg\": %zu, \"echo\": %zu, \"offsets\": [%zu, %zu, %zu, %zu, %zu, %zu], \"cfg_bytes\": [", sizeof c, sizeof e,
           offsetof(smol_csum_echo_cfg_t, bcast_v4), offsetof(smol_csum_echo_cfg_t, reserved),
           offsetof(smol_csum_echo_t, frame_len), offsetof(smol_csum_echo_t, data_off),
           offsetof(smol_csum_echo_t, head_len), offsetof(smol_csum_echo_t, flags));
    for (size_t i = 0; i < sizeof c; ++i) printf("%s%u", i ? ", " : "", ((unsigned char*)&c)[i]);
    printf("], \"echo_bytes\": [");
    for (size_t i = 0; i < sizeof e; ++i) printf("%s%u", i ? ", " : "", ((unsigned char*)&e)[i]);
    printf("]}\n");
    return 0;
}
"""


def test_structs_are_8_bytes_in_every_spelling():
    """C (compiled from the header: sizeof, offsetof and the bytes), ctypes and numpy agree on size and field
    order: each struct filled so that its bytes count 1, 2, 3, ... in memory order."""
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "probe.c"), os.path.join(td, "probe")
        with open(src, "w") as f:
            f.write(_C_PROBE)
        subprocess.run([os.environ.get("CC", "cc"), "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", exe, src],
                       check=True)
        c = json.loads(subprocess.run([exe], check=True, capture_output=True, text=True).stdout)
    assert c["cfg"] == 8 and c["echo"] == 8 and c["offsets"] == [0, 4, 0, 4, 6, 7]
    assert c["cfg_bytes"] == list(range(1, 9)) and c["echo_bytes"] == list(range(1, 9))
    assert ctypes.sizeof(_lib.EchoCfgC) == 8 and ctypes.sizeof(_lib.EchoC) == 8 == E.ECHO_DTYPE.itemsize == R.ECHO_DTYPE.itemsize
    cfg = _lib.EchoCfgC((ctypes.c_uint8 * 4)(1, 2, 3, 4), (ctypes.c_uint8 * 4)(5, 6, 7, 8))
    e = _lib.EchoC(0x04030201, 0x0605, 7, 8)
    assert list(bytes(cfg)) == list(range(1, 9)) and list(bytes(e)) == list(range(1, 9))
    assert [(_lib.EchoC.frame_len.offset), _lib.EchoC.data_off.offset, _lib.EchoC.head_len.offset, _lib.EchoC.flags.offset] == [0, 4, 6, 7]
    a = np.frombuffer(bytes(e), dtype=E.ECHO_DTYPE)[0]
    assert (int(a["frame_len"]), int(a["data_off"]), int(a["head_len"]), int(a["flags"])) == (0x04030201, 0x0605, 7, 8)
    assert E.ECHO_DTYPE == R.ECHO_DTYPE
    assert [E.ECHO_DTYPE.fields[k][1] for k in ("frame_len", "data_off", "head_len", "flags")] == [0, 4, 6, 7]


def test_verify_echo_reply_argument_errors():
    L = smoltcp_amd.lib()
    b = _lib.BatchC()
    b.n, b.stride, b.len, b.kind = 1, 64, 64, 1
    caps = _lib.Caps()
    cfg = _lib.EchoCfgC()
    buf = (ctypes.c_uint8 * 64)()
    dst = (ctypes.c_uint8 * 64)()
    st = (ctypes.c_uint8 * 8)()
    raw = (ctypes.c_uint8 * 64)()
    al = (ctypes.addressof(raw) + 15) & ~15  # 16-byte aligned: slots at al, entries at al + 16
    ctx = ctypes.c_void_p(1)  # never dereferenced: every case below fails its argument checks first
    call = getattr(L, NAME)
    B, C, G = ctypes.byref(b), ctypes.byref(caps), ctypes.byref(cfg)
    EINVAL = _lib.SMOL_EINVAL
    for g in (G, None):  # cfg is nullable: the same errors with and without it
        assert call(None, buf, B, C, g, dst, al, st, al + 16, None) == EINVAL  # NULL ctx
        assert call(ctx, buf, B, None, g, dst, al, st, al + 16, None) == EINVAL  # NULL caps
        assert call(ctx, buf, B, C, g, None, al, st, al + 16, None) == EINVAL  # NULL d_dst
        assert call(ctx, buf, B, C, g, dst, None, st, al + 16, None) == EINVAL  # NULL d_slots
        assert call(ctx, buf, B, C, g, dst, al, None, al + 16, None) == EINVAL  # NULL d_status
        assert call(ctx, buf, B, C, g, dst, al, st, None, None) == EINVAL  # NULL d_echo
        assert call(ctx, buf, B, C, g, dst, al + 8, st, al + 16, None) == EINVAL  # d_slots not 16-byte aligned
        assert call(ctx, buf, B, C, g, dst, al, st, al + 20, None) == EINVAL  # d_echo not 8-byte aligned
        assert call(ctx, None, B, C, g, dst, al, st, al + 16, None) == EINVAL  # NULL d_buf
    bad = _lib.Caps()
    bad.icmpv4 = 4
    assert call(ctx, buf, B, ctypes.byref(bad), G, dst, al, st, al + 16, None) == EINVAL  # bad caps value
    bad = _lib.Caps()
    bad.reserved[1] = 1
    assert call(ctx, buf, B, ctypes.byref(bad), G, dst, al, st, al + 16, None) == EINVAL  # bad caps padding
    for i in range(4):  # a non-zero cfg->reserved, with everything else in order
        badcfg = _lib.EchoCfgC()
        badcfg.reserved[i] = 1
        assert call(ctx, buf, B, C, ctypes.byref(badcfg), dst, al, st, al + 16, None) == EINVAL
    b.len = (1 << 30) + 1  # past SMOL_MAX_RECORD_LEN, as verify
    assert call(ctx, buf, B, C, G, dst, al, st, al + 16, None) == _lib.SMOL_ERANGE
    assert L.smol_csum_batch_verify(ctx, buf, B, C, st, None) == _lib.SMOL_ERANGE
    b.len, b.n = 64, 0  # nothing to do: OK whatever the arrays are, nothing launched
    assert call(ctx, None, B, C, None, None, None, None, None, None) == _lib.SMOL_OK
    assert call(ctx, None, B, C, G, None, None, None, None, None) == _lib.SMOL_OK


def _kat_packet(golden):
    for k in golden.get("kat", []):
        if k.get("name") == "icmpv4_echo":
            return bytes.fromhex(k["bytes"])
    return ECHO_PACKET_BYTES


def test_reference_reply_to_the_known_answer_echo_packet(golden):
    """The reference's own echo request (icmpv4.rs:640-671) behind an IPv4 header, bare and in an Ethernet
    frame: echo_ref's reply verifies under the oracle, answers from the request's destination, and its ICMP
    message differs from the request's only in the type and the checksum."""
    msg = _kat_packet(golden)
    assert msg == ECHO_PACKET_BYTES and msg[8:] == ECHO_DATA_BYTES
    src, dst = bytes([192, 168, 1, 1]), bytes([192, 168, 1, 2])
    for kind in (E.KIND_IP, E.KIND_ETH):
        req = P.ipv4(src, dst, 1, msg)
        if kind == E.KIND_ETH:
            req = P.eth(req)
        e = 14 if kind == E.KIND_ETH else 0
        slots = E.make_slots([5], [100])
        st, ent, arena = R.expected([req], [kind], [0], (0, 0, 0, 0, 0), None, slots, 120)
        fl = int(ent[0]["flags"])
        assert fl & R.REQUEST and fl & R.ANSWERED and fl & R.WRITTEN and not fl & R.HOST
        assert not fl & R.SEND and not st[0] & E.ST_ACCEPT  # the request's IPv4 header checksum is still 0
        hl, ln = int(ent[0]["head_len"]), int(ent[0]["frame_len"])
        assert (hl, ln, int(ent[0]["data_off"])) == (e + 28, e + 28 + 4, e + 28)
        reply = bytes(arena[5:5 + ln])
        assert (arena[:5] == R.SENTINEL).all() and (arena[5 + ln:] == R.SENTINEL).all()
        a = np.frombuffer(reply, np.uint8).copy()
        vst = oracle.batch_verify(a, None, 1, ln, ln, kind)
        assert vst[0] & E.ST_ACCEPT and vst[0] & E.ST_IP_VALID and vst[0] & E.ST_L4_VALID
        assert reply[e + 12:e + 16] == dst and reply[e + 16:e + 20] == src
        if e:
            assert reply[0:6] == req[6:12] and reply[6:12] == req[0:6] and reply[12:14] == req[12:14]
        rmsg = reply[e + 20:]
        assert rmsg[0] == 0 and rmsg[1] == 0 and rmsg[4:] == msg[4:] and rmsg[8:] == ECHO_DATA_BYTES
        assert [i for i in range(len(msg)) if rmsg[i] != msg[i]] == [0, 2]  # type 8 -> 0 moves the checksum's high byte
        assert (rmsg[2] << 8 | rmsg[3]) == 0x96FE  # 0x8efe + 0x0800: the type word left the sum
        # with a filled request the reply is to be sent
        full = np.frombuffer(req, np.uint8).copy()
        oracle.batch_emit(full, None, 1, len(req), len(req), kind)
        st2, ent2, arena2 = R.expected([full.tobytes()], [kind], [0], (0, 0, 0, 0, 0), None, slots, 120)
        assert st2[0] & E.ST_ACCEPT and int(ent2[0]["flags"]) == R.REQUEST | R.ANSWERED | R.WRITTEN | R.SEND
        assert np.array_equal(arena2, arena)
        # caps: tx off leaves both fields zero; the data is echoed all the same
        _, ent3, arena3 = R.expected([req], [kind], [0], (1, 0, 0, 3, 0), None, slots, 120)
        r3 = bytes(arena3[5:5 + ln])
        assert r3[e + 10:e + 12] == b"\0\0" and r3[e + 22:e + 24] == b"\0\0" and r3[e + 24:] == reply[e + 24:]
        # a slot one byte short: reported, not written
        _, ent4, arena4 = R.expected([req], [kind], [0], (0, 0, 0, 0, 0), None, E.make_slots([5], [ln - 1]), 120)
        assert int(ent4[0]["flags"]) == R.REQUEST | R.ANSWERED and int(ent4[0]["frame_len"]) == ln and (arena4 == R.SENTINEL).all()


def test_reference_non_requests_have_zero_entries():
    src, dst = bytes([10, 0, 0, 1]), bytes([10, 0, 0, 2])
    pay = bytes(range(24))
    recs = [
        (P.ipv4(src, dst, 1, P.icmp_echo(0, pay)), E.KIND_IP, 0),                # an echo reply
        (P.ipv4(src, dst, 1, bytes([8, 1]) + P.icmp_echo(8, pay)[2:]), E.KIND_IP, 0),  # code 1
        (P.ipv4(src, dst, 17, P.udp(7, 9, pay)), E.KIND_IP, 0),
        (P.ipv4(src, dst, 1, P.icmp_echo(8, pay), flags_frag=0x2000), E.KIND_IP, 0),   # a fragment
        (P.ipv4(src, dst, 1, P.icmp_echo(8, pay)), E.KIND_IP, E.REC_IPHDR_ONLY),
        (P.ipv4(src, dst, 1, P.icmp_echo(8, pay)), E.KIND_RAW, 0),
        (P.eth(P.ipv4(src, dst, 1, P.icmp_echo(8, pay)), 0x0806), E.KIND_ETH, 0),
        (P.ipv4(src, dst, 1, P.icmp_echo(8, b"")[:6]), E.KIND_IP, 0),            # truncated
    ]
    slots = E.make_slots(np.arange(len(recs)) * 100, 100)
    st, ent, arena = R.expected([r for r, _, _ in recs], [k for _, k, _ in recs], [f for _, _, f in recs], (0,) * 5, None,
                                slots, 100 * len(recs))
    assert not ent.view(np.uint8).any() and (arena == R.SENTINEL).all()
