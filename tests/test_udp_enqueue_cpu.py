"""CPU-side checks of verify_udp_enqueue (smol_csum_batch_verify_udp_enqueue): the symbol, the four structs in
their spellings (header, ctypes, numpy), the argument errors that need no device, and tests/udp_enqueue_ref.py,
the model that the GPU tests (tests/test_gpu_udp_enqueue.py) take their expected entries, metadata and ring
bytes from: the reference's own PacketBuffer tests replayed against it
(tests/golden/packet_buffer_kat.json, src/storage/packet_buffer.rs:262-420), the two layouts on frames, and the
byte classes of the arena.  No kernel is launched here."""
import ctypes
import json
import os
import re

import numpy as np

import oracle
import smoltcp_amd
from smoltcp_amd import _lib
from smoltcp_amd import engine as E
from tests import pktgen as P
from tests import udp_enqueue_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "smol_csum_batch_verify_udp_enqueue"
A4, B4 = bytes([10, 1, 2, 3]), bytes([10, 4, 5, 6])
A6, B6 = bytes(range(0x20, 0x30)), bytes(range(0x40, 0x50))


def _header_text():
    with open(os.path.join(ROOT, "include", "smolcsum.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_symbol_declared_exported_and_listed():
    text = _header_text()
    L = smoltcp_amd.lib()
    assert re.search(r"\b%s\s*\(" % NAME, text)
    assert hasattr(L, NAME) and NAME in _lib.ABI_SYMBOLS
    assert re.search(r"#define\s+SMOL_MAX_SOCKET_DGRAMS\s+256u", text) and E.MAX_SOCKET_DGRAMS == 256
    for name, val in (("UDP", 1), ("ENQUEUED", 2), ("FULL", 4), ("PADDED", 8), ("RESTORED", 16)):
        assert int(re.search(r"#define\s+SMOL_URX_%s\s+0x([0-9a-f]+)u" % name, text).group(1), 16) == val
        assert getattr(E, "URX_" + name) == val
    for name in ("PACKET", "PADDING"):
        assert int(re.search(r"#define\s+SMOL_UMETA_%s\s+(\d+)u" % name, text).group(1)) == getattr(E, "UMETA_" + name)
    assert E.UMETA_PACKET != E.UMETA_PADDING and 0 not in (E.UMETA_PACKET, E.UMETA_PADDING)
    assert L.smol_csum_abi_version() == 6  # additive: the version stays


def _header_struct(name):
    """[(bytes per element, field name, elements)] of a typedef struct in the header."""
    body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % name, _header_text()).group(1)
    return [(int(t) // 8, n, int(k or 1)) for t, n, k in re.findall(r"uint(\d+)_t\s+(\w+)(?:\[(\d+)\])?;", body)]


def test_structs_in_every_spelling():
    for cname, nbytes, cstruct, dt in (("smol_csum_udpsock_t", 48, _lib.UdpSockC, E.UDPSOCK_DTYPE),
                                       ("smol_csum_udpmeta_t", 48, _lib.UdpMetaC, E.UDPMETA_DTYPE),
                                       ("smol_csum_udprx_t", 16, _lib.UdpRxC, E.UDPRX_DTYPE),
                                       ("smol_csum_udpsockout_t", 32, _lib.UdpSockOutC, E.UDPSOCKOUT_DTYPE)):
        fields = _header_struct(cname)
        assert sum(sz * k for sz, _, k in fields) == nbytes == ctypes.sizeof(cstruct) == dt.itemsize
        assert [n for _, n, _ in fields] == [n for n, _ in cstruct._fields_] == list(dt.names)
        assert [sz * k for sz, _, k in fields] == [ctypes.sizeof(t) for _, t in cstruct._fields_] \
            == [dt.fields[n][0].itemsize for n in dt.names]
        # every field at the same offset in all three: the kernel addresses them as dwords
        assert [getattr(cstruct, n).offset for n, _ in cstruct._fields_] == [dt.fields[n][1] for n in dt.names]
    s = _lib.UdpSockC(0x0807060504030201, 0x100F0E0D0C0B0A09, 0x14131211, 0x18171615, 0x1C1B1A19, 0x201F1E1D, 0x24232221,
                      0x28272625, 0x2A29, (ctypes.c_uint16 * 3)(0x2C2B, 0x2E2D, 0x302F))
    assert list(bytes(s)) == list(range(1, 49))
    a = np.frombuffer(bytes(s), dtype=E.UDPSOCK_DTYPE)[0]
    assert int(a["meta_first"]) == 0x100F0E0D0C0B0A09 and int(a["meta_len"]) == 0x28272625 and int(a["port"]) == 0x2A29
    m = E.make_udpsocks([5, 1 << 33], [0, 9], 100, 7, [1, 2], 4, 3, 2, [53, 5000])
    assert m.dtype == E.UDPSOCK_DTYPE and m["dst_offset"].tolist() == [5, 1 << 33] and m["meta_first"].tolist() == [0, 9]
    assert m["payload_cap"].tolist() == [100, 100] and m["payload_read"].tolist() == [7, 7] and m["payload_len"].tolist() == [1, 2]
    assert m["meta_cap"].tolist() == [4, 4] and m["meta_read"].tolist() == [3, 3] and m["meta_len"].tolist() == [2, 2]
    assert m["port"].tolist() == [53, 5000] and not m["reserved"].any()


def test_argument_errors_need_no_device():
    L = smoltcp_amd.lib()
    b = _lib.BatchC()
    b.n, b.stride, b.len, b.kind = 4, 64, 64, 1
    caps = _lib.Caps()
    buf = (ctypes.c_uint8 * 256)()
    dst = (ctypes.c_uint8 * 64)()
    st = (ctypes.c_uint8 * 8)()
    raw = (ctypes.c_uint8 * 320)()
    al = (ctypes.addressof(raw) + 15) & ~15  # 16-byte aligned: groups, socks (48 B), meta (2 x 48 B), rx (4 x 16 B), out
    g, sk, mt, rx, out = al, al + 16, al + 64, al + 160, al + 224
    ctx = ctypes.c_void_p(1)  # never dereferenced: every case below fails its argument checks first
    call = getattr(L, NAME)
    B, C = ctypes.byref(b), ctypes.byref(caps)
    EINVAL = _lib.SMOL_EINVAL
    assert call(None, buf, B, g, 1, C, dst, sk, mt, st, rx, out, None) == EINVAL  # NULL ctx
    assert call(None, buf, B, g, 0, C, dst, sk, mt, st, rx, out, None) == EINVAL  # NULL ctx, also with nothing to do
    assert call(ctx, buf, B, g, 1, None, dst, sk, mt, st, rx, out, None) == EINVAL  # NULL caps
    assert call(ctx, buf, B, None, 1, C, dst, sk, mt, st, rx, out, None) == EINVAL  # NULL d_groups
    assert call(ctx, buf, B, g, 1, C, None, sk, mt, st, rx, out, None) == EINVAL  # NULL d_dst
    assert call(ctx, buf, B, g, 1, C, dst, None, mt, st, rx, out, None) == EINVAL  # NULL d_socks
    assert call(ctx, buf, B, g, 1, C, dst, sk, None, st, rx, out, None) == EINVAL  # NULL d_meta
    assert call(ctx, buf, B, g, 1, C, dst, sk, mt, None, rx, out, None) == EINVAL  # NULL d_status
    assert call(ctx, buf, B, g, 1, C, dst, sk, mt, st, None, out, None) == EINVAL  # NULL d_rx
    assert call(ctx, buf, B, g, 1, C, dst, sk, mt, st, rx, None, None) == EINVAL  # NULL d_out
    assert call(ctx, buf, B, g + 8, 1, C, dst, sk, mt, st, rx, out, None) == EINVAL  # d_groups not 16-byte aligned
    assert call(ctx, buf, B, g, 1, C, dst, sk + 8, mt, st, rx, out, None) == EINVAL  # d_socks not 16-byte aligned
    assert call(ctx, buf, B, g, 1, C, dst, sk, mt + 4, st, rx, out, None) == EINVAL  # d_meta not 16-byte aligned
    assert call(ctx, buf, B, g, 1, C, dst, sk, mt, st, rx + 8, out, None) == EINVAL  # d_rx not 16-byte aligned
    assert call(ctx, buf, B, g, 1, C, dst, sk, mt, st, rx, out + 8, None) == EINVAL  # d_out not 16-byte aligned
    bad = _lib.Caps()
    bad.udp = 4
    assert call(ctx, buf, B, g, 1, ctypes.byref(bad), dst, sk, mt, st, rx, out, None) == EINVAL  # bad caps value
    b.len = (1 << 30) + 1  # past SMOL_MAX_RECORD_LEN, as verify
    assert call(ctx, buf, B, g, 1, C, dst, sk, mt, st, rx, out, None) == _lib.SMOL_ERANGE
    assert L.smol_csum_batch_verify(ctx, buf, B, C, st, None) == _lib.SMOL_ERANGE
    b.len = 64  # no groups: OK whatever the arrays are, nothing launched
    assert call(ctx, buf, B, None, 0, C, None, None, None, None, None, None, None) == _lib.SMOL_OK


# ---- the reference's PacketBuffer tests, replayed ----

def test_reference_packet_buffer_tests_replay():
    with open(os.path.join(ROOT, "tests", "golden", "packet_buffer_kat.json")) as f:
        kat = json.load(f)
    assert len(kat["tests"]) == 12
    for t in kat["tests"]:
        pb = R.PacketBuffer(kat["payload_bytes"], kat["metadata_entries"])
        for k, op in enumerate(t["ops"]):
            where = f"{t['name']} (packet_buffer.rs:{t['lines']}) op {k}: {op}"
            if op["op"] == "enqueue":
                res, ring_off = pb.enqueue(op["size"])[:2]
                assert ("ok" if res & R.OK else "full") == op["result"], where
                if "data" in op:
                    assert res & R.OK and len(op["data"]) == op["size"], where
                    pb.write(ring_off, op["data"].encode())
            elif op["op"] == "dequeue":
                got = pb.dequeue()
                want = op["result"]
                if want == "empty":
                    assert got is None, where
                elif want == "ok":
                    assert got is not None, where
                elif isinstance(want, int):
                    assert got is not None and len(got) == want, where
                else:
                    assert got == want.encode(), where
            elif op["op"] == "dequeue_with_err":
                pb.dequeue_padding()
                assert pb.ml > 0, where
            elif op["op"] == "peek":
                got = pb.peek()
                assert (got is None) if op["result"] == "empty" else got == op["result"].encode(), where
            elif op["op"] == "meta_len":
                assert pb.ml == op["result"], where
            elif op["op"] == "is_empty":
                assert (pb.ml == 0) == op["result"], where
            elif op["op"] == "is_full":
                assert (pb.ml == pb.M) == op["result"], where
            else:
                raise AssertionError(where)
            assert pb.valid(), where
    # the last test's enqueue took the padding entry and then found no room: PADDED and FULL together
    pb = R.PacketBuffer(16, 4)
    for size in (12, 1, 1, 1):
        assert pb.enqueue(size)[0] == R.OK
    assert len(pb.dequeue()) == 12
    assert pb.enqueue(5) == (R.PADDED | R.FULL, 0, 0, 0, 1) and pb.state() == (12, 4, 1, 4)


# ---- the call on frames ----

def _frames(payloads, dport=5000, v6=()):
    recs = []
    for j, p in enumerate(payloads):
        u = P.udp(4000 + j, dport, p)
        recs.append(P.eth(P.ipv6(A6, B6, 17, u), 0x86DD) if j in v6 else P.eth(P.ipv4(A4, B4, 17, u)))
    return recs


def _expected(recs, groups, socks, flips=(), caps=(0, 0, 0, 0, 0), arena=256, meta=16):
    buf, offs, lens = P.pack(recs, gap_rng=np.random.default_rng(3))
    kinds = np.full(len(recs), E.KIND_ETH, np.uint8)
    desc = E.make_descriptors(offs, lens, kinds)
    oracle.batch_emit(buf, desc, len(recs))
    for i, o, bit in flips:
        buf[int(offs[i]) + o] ^= 1 << bit
    st = oracle.batch_verify(buf.copy(), desc, len(recs), caps=caps)
    placed = [bytes(buf[int(o):int(o) + int(n)]) for o, n in zip(offs, lens)]
    return R.expected(placed, kinds, np.zeros(len(recs), np.uint8), groups, socks, st, arena, meta), placed


def test_expected_on_frames_two_layouts():
    rng = np.random.default_rng(5)
    pay = [P.rand_bytes(rng, n) for n in (30, 40, 50)]
    recs = _frames(pay, v6={2})
    socks = E.make_udpsocks([10], [2], 160, 110, 2, 8, 6, 1, 5000)
    # every candidate accepted: 30 @112; 40: contig 18 -> PADDING(18) at metadata index 0 (7 + 1 wraps), @0; 50 @40
    exp, placed = _expected(recs, [(0, 3, 0)], socks)
    rx, out = exp["rx"], exp["outs"][0]
    assert rx["flags"].tolist() == [3, 3 | E.URX_PADDED, 3] and rx["ring_off"].tolist() == [112, 0, 40]
    assert rx["meta_idx"].tolist() == [7, 1, 2] and rx["len"].tolist() == [30, 40, 50] and rx["off"].tolist() == [42, 42, 62]
    assert tuple(out)[:7] == (110, 2 + 30 + 18 + 40 + 50, 6, 5, 3, 0, 0) and int(out["valid"]) == 1
    assert np.nonzero(exp["meta_written"])[0].tolist() == [2, 3, 4, 9]
    pad, last = exp["meta"][2], exp["meta"][4]
    assert (int(pad["size"]), int(pad["kind"])) == (18, E.UMETA_PADDING) and not pad["remote_addr"].any() and int(pad["record"]) == 0
    assert (int(last["size"]), int(last["record"]), int(last["src_port"]), int(last["family"]), int(last["kind"])) == \
        (50, 2, 4002, 6, E.UMETA_PACKET)
    assert bytes(last["remote_addr"]) == A6 and bytes(last["local_addr"]) == B6
    assert bytes(exp["meta"][9]["remote_addr"]) == A4 + bytes(12) and bytes(exp["meta"][9]["local_addr"]) == B4 + bytes(12)
    assert bytes(exp["arena"][10 + 112:10 + 142]) == pay[0] and bytes(exp["arena"][10:10 + 40]) == pay[1]
    assert exp["spec_only"].sum() == 0 and (exp["arena"] != R.SENTINEL).sum() <= 120
    # the first one corrupted: it takes no space.  40 @112, 50: contig 8 -> PADDING(8), @0; both moved
    exp, _ = _expected(recs, [(0, 3, 0)], socks, flips=[(0, 50, 1)])
    rx = exp["rx"]
    assert rx["flags"].tolist() == [1, 3 | E.URX_RESTORED, 3 | E.URX_RESTORED | E.URX_PADDED] and rx["ring_off"].tolist() == [0, 112, 0]
    assert int(exp["outs"][0]["restored"]) == 2 and int(exp["outs"][0]["payload_len"]) == 2 + 40 + 8 + 50
    # bytes only the speculative layout covers: 30's speculative place @112..142 lies inside 40's accepted one @112..152 and
    # 40's @0..40 inside 50's accepted one @0..50; 50's speculative place @40..90 reaches past it
    only = np.nonzero(exp["spec_only"])[0] - 10
    assert only.tolist() == list(range(50, 90))
    got = exp["arena"].copy()
    assert R.check_arena(got, exp).size == 0
    got[10 + 60] = exp["spec_arena"][10 + 60]  # a speculative byte left in free space: allowed
    assert R.check_arena(got, exp).size == 0
    got[10 + 60] ^= 0xFF  # any other value there is not
    assert R.check_arena(got, exp).tolist() == [70]
    got = exp["arena"].copy()
    got[10 + 100] = 1  # free space no layout covers
    got[5] = 1  # outside the ring
    assert R.check_arena(got, exp).tolist() == [5, 110]


def test_expected_port_mismatch_and_invalid_groups():
    rng = np.random.default_rng(6)
    recs = _frames([P.rand_bytes(rng, 8) for _ in range(4)]) + _frames([P.rand_bytes(rng, 8)], dport=5001)
    socks = E.make_udpsocks([0, 64, 128, 192], [0, 4, 8, 12], 64, 0, [0, 65, 0, 0], 4, [0, 0, 4, 0], 0, 5000)
    socks["reserved"][3] = (0, 1, 0)
    exp, _ = _expected(recs, [(3, 2, 0), (0, 1, 0), (1, 1, 0), (2, 1, 0)], socks)
    assert exp["outs"]["valid"].tolist() == [1, 0, 0, 0] and exp["written"].tolist() == [False, False, False, True, True]
    assert exp["rx"]["flags"].tolist() == [0, 0, 0, 3, 0] and not exp["rx"][4].tobytes().strip(b"\0")
