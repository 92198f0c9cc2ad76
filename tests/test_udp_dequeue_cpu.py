"""CPU-side checks of udp_dequeue_emit (smol_csum_batch_udp_dequeue_emit): the symbol, the three structs in their
spellings (header, ctypes, numpy), the argument errors that need no device, and tests/udp_dequeue_ref.py, the model
that the GPU tests (tests/test_gpu_udp_dequeue.py) take their expected entries and frames from: the reference's own
PacketBuffer tests replayed against its walk (tests/golden/packet_buffer_kat.json,
src/storage/packet_buffer.rs:262-420), its frames against the oracle's verify, and a ring filled by the enqueue
model drained by it.  No kernel is launched here."""
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
from tests import udp_dequeue_ref as D
from tests import udp_enqueue_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "smol_csum_batch_udp_dequeue_emit"
A4, B4 = bytes([10, 1, 2, 3]), bytes([10, 4, 5, 6])
A6, B6 = bytes(range(0x20, 0x30)), bytes(range(0x40, 0x50))
ETH = (bytes([2, 0, 0, 0, 0, 9]), bytes([2, 0, 0, 0, 0, 7]))


def _header_text():
    with open(os.path.join(ROOT, "include", "smolcsum.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_symbol_declared_exported_and_listed():
    text = _header_text()
    L = smoltcp_amd.lib()
    assert re.search(r"\b%s\s*\(" % NAME, text)
    assert hasattr(L, NAME) and NAME in _lib.ABI_SYMBOLS
    for name, val in (("SENT", 1), ("OVERSIZE", 2), ("PADDED", 4)):
        assert int(re.search(r"#define\s+SMOL_UTX_%s\s+0x([0-9a-f]+)u" % name, text).group(1), 16) == val == getattr(E, "UTX_" + name)
    for name, val in (("EMPTY", 1), ("MAX", 2), ("NOSPACE", 3), ("CORRUPT", 4)):
        assert int(re.search(r"#define\s+SMOL_UTX_STOP_%s\s+(\d+)u" % name, text).group(1)) == val == getattr(E, "UTX_STOP_" + name)
    assert int(re.search(r"#define\s+SMOL_UTXS_ETH\s+0x([0-9a-f]+)u", text).group(1), 16) == E.UTXS_ETH == 1
    assert L.smol_csum_abi_version() == 6  # additive: the version stays


def _header_struct(name):
    """[(bytes per element, field name, elements)] of a typedef struct in the header."""
    body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % name, _header_text()).group(1)
    return [(int(t) // 8, n, int(k or 1)) for t, n, k in re.findall(r"uint(\d+)_t\s+(\w+)(?:\[(\d+)\])?;", body)]


def test_structs_in_every_spelling():
    for cname, nbytes, cstruct, dt in (("smol_csum_udptxsock_t", 96, _lib.UdpTxSockC, E.UDPTXSOCK_DTYPE),
                                       ("smol_csum_udptx_t", 16, _lib.UdpTxC, E.UDPTX_DTYPE),
                                       ("smol_csum_udptxout_t", 32, _lib.UdpTxOutC, E.UDPTXOUT_DTYPE)):
        fields = _header_struct(cname)
        assert sum(sz * k for sz, _, k in fields) == nbytes == ctypes.sizeof(cstruct) == dt.itemsize
        assert [n for _, n, _ in fields] == [n for n, _ in cstruct._fields_] == list(dt.names)
        assert [sz * k for sz, _, k in fields] == [ctypes.sizeof(t) for _, t in cstruct._fields_] \
            == [dt.fields[n][0].itemsize for n in dt.names]
        # every field at the same offset in all three: the kernel addresses them as dwords and bytes
        assert [getattr(cstruct, n).offset for n, _ in cstruct._fields_] == [dt.fields[n][1] for n in dt.names]
    assert E.UDPTXSOCK_DTYPE.fields["eth_dst"][1] == 70 and E.UDPTXSOCK_DTYPE.fields["reserved"][1] == 82
    m = E.make_udptxsocks([5, 1 << 33], [0, 9], [7, 1 << 34], [0, 3], 100, 7, [1, 2], 4, 3, 2, 4000, [1, 256], 53, 1500,
                          hop_limits=[1, 255], eth=ETH)
    assert m.dtype == E.UDPTXSOCK_DTYPE and m["src_offset"].tolist() == [5, 1 << 33] and m["dst_offset"].tolist() == [7, 1 << 34]
    assert m["meta_first"].tolist() == [0, 9] and m["tx_first"].tolist() == [0, 3] and m["payload_len"].tolist() == [1, 2]
    assert m["dst_cap"].tolist() == [4000, 4000] and m["max_dgrams"].tolist() == [1, 256] and m["hop_limit"].tolist() == [1, 255]
    assert m["flags"].tolist() == [1, 1] and bytes(m["eth_dst"][1]) == ETH[0] and bytes(m["eth_src"][0]) == ETH[1]
    assert not m["reserved"].any()
    assert not E.make_udptxsocks([0], 0, 0, 0, 1, 0, 0, 1, 0, 0, 1, 1, 1, 1)["flags"].any()


def test_argument_errors_need_no_device():
    L = smoltcp_amd.lib()
    caps = _lib.Caps()
    src = (ctypes.c_uint8 * 64)()
    dst = (ctypes.c_uint8 * 64)()
    raw = (ctypes.c_uint8 * 320)()
    al = (ctypes.addressof(raw) + 15) & ~15  # 16-byte aligned: socks (96 B), meta (48 B), tx (2 x 16 B), out (32 B)
    sk, mt, tx, out = al, al + 96, al + 144, al + 176
    ctx = ctypes.c_void_p(1)  # never dereferenced: every case below fails its argument checks first
    call = getattr(L, NAME)
    C = ctypes.byref(caps)
    EINVAL = _lib.SMOL_EINVAL
    assert call(None, src, sk, 1, mt, C, dst, 0, tx, out, None) == EINVAL  # NULL ctx
    assert call(None, src, sk, 0, mt, C, dst, 0, tx, out, None) == EINVAL  # NULL ctx, also with nothing to do
    assert call(ctx, src, sk, 1, mt, None, dst, 0, tx, out, None) == EINVAL  # NULL caps
    assert call(ctx, None, sk, 1, mt, C, dst, 0, tx, out, None) == EINVAL  # NULL d_src
    assert call(ctx, src, None, 1, mt, C, dst, 0, tx, out, None) == EINVAL  # NULL d_socks
    assert call(ctx, src, sk, 1, None, C, dst, 0, tx, out, None) == EINVAL  # NULL d_meta
    assert call(ctx, src, sk, 1, mt, C, None, 0, tx, out, None) == EINVAL  # NULL d_dst
    assert call(ctx, src, sk, 1, mt, C, dst, 0, None, out, None) == EINVAL  # NULL d_tx
    assert call(ctx, src, sk, 1, mt, C, dst, 0, tx, None, None) == EINVAL  # NULL d_out
    assert call(ctx, src, sk + 8, 1, mt, C, dst, 0, tx, out, None) == EINVAL  # d_socks not 16-byte aligned
    assert call(ctx, src, sk, 1, mt + 4, C, dst, 0, tx, out, None) == EINVAL  # d_meta not 16-byte aligned
    assert call(ctx, src, sk, 1, mt, C, dst, 0, tx + 8, out, None) == EINVAL  # d_tx not 16-byte aligned
    assert call(ctx, src, sk, 1, mt, C, dst, 0, tx, out + 8, None) == EINVAL  # d_out not 16-byte aligned
    bad = _lib.Caps()
    bad.udp = 4
    assert call(ctx, src, sk, 1, mt, ctypes.byref(bad), dst, 0, tx, out, None) == EINVAL  # bad caps value
    bad = _lib.Caps()
    bad.reserved[1] = 1
    assert call(ctx, src, sk, 0, mt, ctypes.byref(bad), dst, 0, tx, out, None) == EINVAL  # bad caps, also with nothing to do
    # no groups: OK whatever the arrays are, nothing launched
    assert call(ctx, None, None, 0, None, C, None, 1536, None, None, None) == _lib.SMOL_OK


# ---- the reference's PacketBuffer tests, replayed against the model's walk ----

def test_reference_packet_buffer_tests_replay():
    with open(os.path.join(ROOT, "tests", "golden", "packet_buffer_kat.json")) as f:
        kat = json.load(f)
    seen = {"dequeue": 0, "dequeue_with_err": 0}
    for t in kat["tests"]:
        pb = R.PacketBuffer(kat["payload_bytes"], kat["metadata_entries"])
        for k, op in enumerate(t["ops"]):
            where = f"{t['name']} (packet_buffer.rs:{t['lines']}) op {k}: {op}"
            if op["op"] == "enqueue":
                res, ring_off = pb.enqueue(op["size"])[:2]
                assert ("ok" if res & R.OK else "full") == op["result"], where
                if "data" in op:
                    pb.write(ring_off, op["data"].encode())
            elif op["op"] == "dequeue":
                seen["dequeue"] += 1
                res, ring_off, _, size, _ = D.dequeue(pb)
                want = op["result"]
                if want == "empty":
                    assert res & D.EMPTY and not res & D.OK, where
                else:
                    assert res & D.OK, where
                    got = bytes(pb.store[ring_off:ring_off + size])
                    if isinstance(want, int):
                        assert size == want, where
                    elif want != "ok":
                        assert got == want.encode(), where
            elif op["op"] == "dequeue_with_err":  # the closure fails: the padding is gone, the packet stays
                seen["dequeue_with_err"] += 1
                before = pb.ml
                res, _, meta_idx, _, _ = D.front(pb)
                assert res & D.OK and meta_idx == pb.mr and pb.ml == before - (1 if res & D.PADDED else 0) and pb.ml > 0, where
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
    assert seen["dequeue"] > 10 and seen["dequeue_with_err"] >= 1


# ---- the model on rings ----

def _ring(payloads, P_=512, M=16, pr=0, mr=0, fams=None, dports=None, base=3, mfirst=1):
    """A transmit ring filled by the enqueue model: (src arena, meta array, (pr, pl, mr, ml)).  pr > 0: a datagram
    of pr bytes is enqueued first and dequeued once the first payload is in (an empty ring resets its read index)."""
    pb = R.PacketBuffer(P_, M, 0, 0, mr, 0)
    src = np.random.default_rng(9).integers(0, 256, base + P_ + 5, dtype=np.uint8)
    meta = np.zeros(mfirst + M + 1, E.UDPMETA_DTYPE)
    meta.view(np.uint8)[:] = 0x5A
    if pr:
        assert pb.enqueue(pr)[0] == R.OK
    for j, p in enumerate(payloads):
        res, at, mi, pad_idx, pad_size = pb.enqueue(len(p))
        if pr and j == 0:
            assert len(pb.dequeue()) == pr
        assert res & R.OK, (j, res)
        if res & R.PADDED:
            e = np.zeros(1, E.UDPMETA_DTYPE)[0]
            e["size"], e["kind"] = pad_size, E.UMETA_PADDING
            meta[mfirst + pad_idx] = e
        fam = fams[j] if fams else 4
        e = np.zeros(1, E.UDPMETA_DTYPE)[0]
        e["size"], e["src_port"], e["family"], e["kind"] = len(p), (dports[j] if dports else 7000 + j), fam, E.UMETA_PACKET
        a, b = (A4, B4) if fam == 4 else (A6, B6)
        e["remote_addr"][:len(a)] = np.frombuffer(a, np.uint8)
        e["local_addr"][:len(b)] = np.frombuffer(b, np.uint8)
        meta[mfirst + mi] = e
        src[base + at:base + at + len(p)] = np.frombuffer(p, np.uint8)
    return src, meta, pb.state()


def test_model_frames_pass_verify_and_carry_the_payloads():
    rng = np.random.default_rng(4)
    pay = [P.rand_bytes(rng, n) for n in (1, 0, 17, 200, 33, 150)]
    # 200 wraps: a padding entry in the middle (pr 400: 1 @400, 0 @401, 17 @401, 200: contig 94 -> padding, @0)
    src, meta, st = _ring(pay, pr=400, fams=[4, 6, 4, 6, 4, 6])
    for eth in (None, ETH):
        socks = E.make_udptxsocks([3], 1, 11, 2, 512, st[0], st[1], 16, st[2], st[3], 4000, 256, 5353, 1500, hop_limits=9, eth=eth)
        exp = D.expected(src, socks, meta, (0, 0, 0, 0, 0), 0, 4100, 16)
        out = exp["outs"][0]
        assert (int(out["sent"]), int(out["oversize"]), int(out["stop"]), int(out["valid"])) == (6, 0, E.UTX_STOP_EMPTY, 1)
        assert (int(out["payload_len"]), int(out["meta_len"])) == (0, 0)
        assert exp["tx_written"].tolist() == [False] * 2 + [True] * 6 + [False] * 8
        assert exp["tx"]["flags"][2:8].tolist() == [1, 1, 1, 1 | E.UTX_PADDED, 1, 1] and exp["tx"]["ring_off"][5] == 0
        io = 14 if eth else 0
        frames = [f for _, _, _, f in exp["frames"]]
        assert [len(f) for f in frames] == [io + (28 if k % 2 == 0 else 48) + len(p) for k, p in enumerate(pay)]
        assert int(out["bytes"]) == sum(len(f) for f in frames)
        assert [f[len(f) - len(p):] for f, p in zip(frames, pay) if p] == [p for p in pay if p]
        buf, offs, lens = P.pack(frames)
        kinds = np.full(len(frames), E.KIND_ETH if eth else E.KIND_IP, np.uint8)
        vst = oracle.batch_verify(buf, E.make_descriptors(offs, lens, kinds), len(frames))
        assert (vst & E.ST_ACCEPT).all() and (vst & E.ST_L4_VALID).all() and (vst & E.ST_IP_VALID).all()
        f0 = frames[0][io:]
        assert f0[:2] == b"\x45\x00" and f0[4:10] == bytes([0, 0, 0x40, 0, 9, 17]) and f0[12:16] == B4 and f0[16:20] == A4
        assert f0[20:24] == P.be16(5353) + P.be16(7000)
        if eth:
            assert frames[1][:14] == ETH[0] + ETH[1] + b"\x86\xdd"
    # caps that fill nothing: both fields are 0
    exp = D.expected(src, socks, meta, (3, 3, 0, 0, 0), 0, 4100, 16)
    f0 = exp["frames"][0][3]
    assert f0[14 + 10:14 + 12] == b"\0\0" and f0[14 + 26:14 + 28] == b"\0\0"


def test_model_stops_and_oversize():
    rng = np.random.default_rng(5)
    pay = [P.rand_bytes(rng, n) for n in (100, 300, 50)]
    src, meta, st = _ring(pay)
    mk = lambda **k: E.make_udptxsocks([3], 1, 0, 0, 512, st[0], st[1], 16, st[2], st[3], k.get("cap", 4000), k.get("maxd", 256),
                                       9, k.get("mtu", 1500))
    # OVERSIZE in the middle: dequeued, no frame, the next frame's place not advanced
    exp = D.expected(src, mk(mtu=200), meta, (0, 0, 0, 0, 0), 0, 4000, 4)
    assert exp["tx"]["flags"].tolist() == [1, 2, 1, 0] and exp["tx"]["frame_off"].tolist() == [0, 128, 128, 0]
    assert exp["tx"]["ip_len"].tolist() == [128, 0, 78, 0] and exp["tx"]["ring_off"].tolist() == [0, 100, 400, 0]
    assert (int(exp["outs"][0]["oversize"]), int(exp["outs"][0]["bytes"])) == (1, 206)
    # NOSPACE at frame 1 through dst_cap: it stays queued
    exp = D.expected(src, mk(cap=128 + 327), meta, (0, 0, 0, 0, 0), 0, 4000, 4)
    o = exp["outs"][0]
    assert (int(o["sent"]), int(o["stop"]), int(o["meta_len"]), int(o["payload_len"]), int(o["payload_read"])) == \
        (1, E.UTX_STOP_NOSPACE, 2, 350, 100)
    # ... and through the stride
    exp = D.expected(src, mk(), meta, (0, 0, 0, 0, 0), 327, 4000, 4)
    assert int(exp["outs"][0]["stop"]) == E.UTX_STOP_NOSPACE and int(exp["outs"][0]["bytes"]) == 327
    exp = D.expected(src, mk(), meta, (0, 0, 0, 0, 0), 328, 4000, 4)
    assert int(exp["outs"][0]["stop"]) == E.UTX_STOP_EMPTY and exp["tx"]["frame_off"].tolist() == [0, 328, 656, 0]
    # MAX
    exp = D.expected(src, mk(maxd=2), meta, (0, 0, 0, 0, 0), 0, 4000, 4)
    assert (int(exp["outs"][0]["stop"]), int(exp["outs"][0]["meta_len"])) == (E.UTX_STOP_MAX, 1)
    # CORRUPT: a bad kind, a bad family, a size past the ring's contiguous bytes
    for field, val in (("kind", 0), ("kind", 3), ("family", 5), ("size", 413)):
        m2 = meta.copy()
        m2[1 + 1][field] = val
        o = D.expected(src, mk(), m2, (0, 0, 0, 0, 0), 0, 4000, 4)["outs"][0]
        assert (int(o["sent"]), int(o["stop"]), int(o["meta_len"])) == (1, E.UTX_STOP_CORRUPT, 2), (field, val)
    # an invalid group: all zero
    s = mk()
    s["reserved"][0][13] = 1
    exp = D.expected(src, s, meta, (0, 0, 0, 0, 0), 0, 4000, 4)
    assert not exp["outs"].view(np.uint8).any() and not exp["tx_written"].any() and (exp["arena"] == D.SENTINEL).all()


def test_enqueue_model_then_dequeue_model_returns_the_payloads_in_order():
    rng = np.random.default_rng(6)
    for pr, mr in ((0, 0), (100, 3), (250, 7)):
        pay = [P.rand_bytes(rng, int(n)) for n in rng.integers(0, 40, 7)]
        src, meta, st = _ring(pay, P_=300, M=8, pr=pr, mr=mr)
        socks = E.make_udptxsocks([3], 1, 0, 0, 300, st[0], st[1], 8, st[2], st[3], 1 << 20, 256, 9, 1500)
        pb = D.load(socks[0], meta)
        got = []
        while True:
            res, ring_off, _, size, _ = D.dequeue(pb, D.meta_kind)
            if not res & D.OK:
                assert res & D.EMPTY
                break
            got.append(bytes(src[3 + ring_off:3 + ring_off + size]))
        assert got == pay and pb.pl == 0 and pb.ml == 0
