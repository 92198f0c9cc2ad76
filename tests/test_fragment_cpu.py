"""CPU-side checks of fragment_emit (smol_csum_batch_fragment_emit): the symbol, the plan and result
structs in their three spellings (header, ctypes, numpy), the argument errors that need no device, and
tests/fragment_ref.py, the numpy restatement of the cut that the GPU tests (tests/test_gpu_fragment.py)
take their expected entries and destination bytes from.  No kernel is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest

import oracle
import smoltcp_amd
from smoltcp_amd import _lib
from smoltcp_amd import engine as E
from tests import fragment_ref as C
from tests import pktgen as P
from tests import reassemble_ref as R
from tests import test_frag_cpu as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "smol_csum_batch_fragment_emit"


def test_symbol_declared_exported_and_listed():
    with open(os.path.join(ROOT, "include", "smolcsum.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    L = smoltcp_amd.lib()
    assert re.search(r"\b%s\s*\(" % NAME, text)
    assert hasattr(L, NAME) and NAME in _lib.ABI_SYMBOLS
    assert "smol_csum_fragplan_t" in text and "smol_csum_fragout_t" in text
    assert L.smol_csum_abi_version() == 6  # additive: the version stays


def _header_struct(name):
    with open(os.path.join(ROOT, "include", "smolcsum.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % name, text).group(1)
    return [(t, n) for t, n in re.findall(r"(uint\d+_t)\s+(\w+);", body)]


def test_structs_are_16_bytes_in_every_spelling():
    size = {"uint8_t": 1, "uint16_t": 2, "uint32_t": 4, "uint64_t": 8}
    for cname, cstruct, dts in (("smol_csum_fragplan_t", _lib.FragPlanC, (E.FRAGPLAN_DTYPE, C.FRAGPLAN_DTYPE)),
                                ("smol_csum_fragout_t", _lib.FragOutC, (E.FRAGOUT_DTYPE, C.FRAGOUT_DTYPE))):
        fields = _header_struct(cname)
        assert sum(size[t] for t, _ in fields) == 16 == ctypes.sizeof(cstruct)
        assert [n for _, n in fields] == [n for n, _ in cstruct._fields_] == list(dts[0].names)
        assert [size[t] for t, _ in fields] == [ctypes.sizeof(t) for _, t in cstruct._fields_]
        assert dts[0] == dts[1] and dts[0].itemsize == 16
    p = _lib.FragPlanC(0x0807060504030201, 0x0C0B0A09, 0x0E0D, 0x100F)
    assert list(bytes(p)) == list(range(1, 17))
    a = np.frombuffer(bytes(p), dtype=E.FRAGPLAN_DTYPE)[0]
    assert (int(a["dst_offset"]), int(a["cap"]), int(a["ip_mtu"]), int(a["ident"])) == \
        (0x0807060504030201, 0x0C0B0A09, 0x0E0D, 0x100F)
    o = _lib.FragOutC(0x04030201, 0x08070605, 0x0C0B0A09, 13, 14, 0x100F)
    assert list(bytes(o)) == list(range(1, 17))
    a = np.frombuffer(bytes(o), dtype=E.FRAGOUT_DTYPE)[0]
    assert (int(a["count"]), int(a["frame_len"]), int(a["last_len"]), int(a["status"]), int(a["written"]),
            int(a["reserved"])) == (0x04030201, 0x08070605, 0x0C0B0A09, 13, 14, 0x100F)
    m = E.make_fragplans([5, 9], [100, 200], 576, [7, 8])
    assert m.dtype == E.FRAGPLAN_DTYPE and m["ip_mtu"].tolist() == [576, 576] and m["ident"].tolist() == [7, 8]
    assert m["dst_offset"].tolist() == [5, 9] and m["cap"].tolist() == [100, 200]


def test_argument_errors_need_no_device():
    L = smoltcp_amd.lib()
    b = _lib.BatchC()
    b.n, b.stride, b.len, b.kind = 4, 64, 64, 1
    caps = _lib.Caps()
    buf = (ctypes.c_uint8 * 256)()
    dst = (ctypes.c_uint8 * 64)()
    raw = (ctypes.c_uint8 * 160)()
    al = (ctypes.addressof(raw) + 15) & ~15  # 16-byte aligned: plans at al, out at al + 64
    pl, out = al, al + 64
    ctx = ctypes.c_void_p(1)  # never dereferenced: every case below fails its argument checks first
    call = getattr(L, NAME)
    B, Cp = ctypes.byref(b), ctypes.byref(caps)
    EINVAL = _lib.SMOL_EINVAL
    assert call(None, buf, B, Cp, dst, pl, 0, out, None) == EINVAL  # NULL ctx
    b.n = 0
    assert call(None, buf, B, Cp, dst, pl, 0, out, None) == EINVAL  # NULL ctx, also with nothing to do
    b.n = 4
    assert call(ctx, buf, B, None, dst, pl, 0, out, None) == EINVAL  # NULL caps
    assert call(ctx, buf, B, Cp, None, pl, 0, out, None) == EINVAL  # NULL d_dst
    assert call(ctx, buf, B, Cp, dst, None, 0, out, None) == EINVAL  # NULL d_plans
    assert call(ctx, buf, B, Cp, dst, pl, 0, None, None) == EINVAL  # NULL d_out
    assert call(ctx, buf, B, Cp, dst, pl + 8, 0, out, None) == EINVAL  # d_plans not 16-byte aligned
    assert call(ctx, buf, B, Cp, dst, pl, 0, out + 4, None) == EINVAL  # d_out not 16-byte aligned
    bad = _lib.Caps()
    bad.ipv4 = 4
    assert call(ctx, buf, B, ctypes.byref(bad), dst, pl, 0, out, None) == EINVAL  # bad caps value
    b.len = (1 << 30) + 1  # past SMOL_MAX_RECORD_LEN, as emit
    assert call(ctx, buf, B, Cp, dst, pl, 0, out, None) == _lib.SMOL_ERANGE
    assert L.smol_csum_batch_emit(ctx, buf, B, Cp, None, None) == _lib.SMOL_ERANGE
    b.len, b.n = 64, 0  # no records: OK whatever the arrays are, nothing launched
    assert call(ctx, None, B, Cp, None, None, 0, None, None) == _lib.SMOL_OK


def _plans_back_to_back(recs, kind, mtu, stride, start=3):
    """Plans with every datagram's exact need as its cap, slots one after the other from an odd offset."""
    need = C.expected(recs, [kind] * len(recs), [0] * len(recs), E.make_fragplans([0] * len(recs), 0, mtu, 0), stride,
                      F.DEFAULT, 1)[0]
    offs, pos = [], start
    for e in need:
        S = stride or int(e["frame_len"])
        offs.append(pos)
        pos += (int(e["count"]) - 1) * S + int(e["last_len"])
    return E.make_fragplans(offs, [b - a for a, b in zip(offs, offs[1:] + [pos])], mtu, 0x4000 + np.arange(len(recs))), pos


@pytest.mark.parametrize("eth", [False, True])
@pytest.mark.parametrize("mtu", [28, 68, 576, 1500])
def test_helper_cuts_what_the_builders_cut_and_reassembly_returns_it(mtu, eth):
    """The helper's frames for F.datagrams equal F.tx_pair's reference fragments; oracle.batch_verify_frag
    accepts every one of them; tests.reassemble_ref puts the emitted payload back together; the sentinel
    survives outside the frames."""
    rng = np.random.default_rng(mtu + eth)
    small = mtu <= 68
    dgs = F.datagrams(rng, 8, 60 if small else 1600, 300 if small else 5000)
    _, ref, groups = F.tx_pair(dgs, mtu, eth)
    kind = E.KIND_ETH if eth else E.KIND_IP
    io = 14 if eth else 0
    recs = [P.eth(d) if eth else d for d in dgs]
    stride = io + mtu + 3
    plans, end = _plans_back_to_back(recs, kind, mtu, stride)
    out, arena = C.expected(recs, [kind] * len(recs), [0] * len(recs), plans, stride, F.DEFAULT, end + 9)
    frames = []
    covered = np.zeros(arena.size, bool)
    for i, (first, count) in enumerate(groups):
        assert (int(out[i]["count"]), int(out[i]["written"]), int(out[i]["status"])) == (count, 1, 0)
        assert int(out[i]["frame_len"]) == len(ref[first]) and int(out[i]["last_len"]) == len(ref[first + count - 1])
        for k in range(count):
            o = int(plans[i]["dst_offset"]) + k * stride
            ln = int(out[i]["frame_len"] if k + 1 < count else out[i]["last_len"])
            assert arena[o:o + ln].tobytes() == ref[first + k]
            frames.append(arena[o:o + ln].tobytes())
            covered[o:o + ln] = True
    assert (arena[~covered] == C.SENTINEL).all()
    # the frames are verify_reassemble's input
    buf, offs, lens, _, g = F.pack(frames, groups)
    desc = P.oracle_desc(offs, lens, kind)
    assert (oracle.batch_verify_frag(buf, desc, len(desc), g) & F.ST_ACCEPT).all()
    T = [len(d) - 20 for d in dgs]
    dg, back = R.expected(frames, [kind] * len(frames), [0] * len(frames), [(f, c, 0) for f, c in groups],
                          np.cumsum([0] + T[:-1]), T, sum(T))
    pos = 0
    for d, e in zip(dgs, dg):
        want = F.emit_whole(d, F.DEFAULT)[20:]
        assert int(e["len"]) == len(want) and e["copied"] == 1 and back[pos:pos + len(want)].tobytes() == want
        pos += len(want)


def test_helper_rules():
    rng = np.random.default_rng(3)
    d = P.ipv4(F.A, F.B, 17, P.udp(7, 9, P.rand_bytes(rng, 992)))  # T = 1000
    one = lambda rec, kind=E.KIND_IP, mtu=576, cap=1 << 20, stride=0, flags=0, caps=F.DEFAULT: C.expected(  # noqa: E731
        [rec], [kind], [flags], E.make_fragplans([2], cap, mtu, 0x1234), stride, caps, 4000)
    out, arena = one(d)
    assert (int(out[0]["count"]), int(out[0]["frame_len"]), int(out[0]["last_len"]), int(out[0]["written"])) == (2, 572, 468, 1)
    assert (arena[:2] == C.SENTINEL).all() and (arena[2 + 572 + 468:] == C.SENTINEL).all()
    assert arena[2 + 4:2 + 6].tobytes() == b"\x12\x34" and arena[2 + 6] == 0x20  # the plan's ident, MF, DF cleared
    # one frame: the record emitted, ident and DF as the caller wrote them
    out, arena = one(d, mtu=1020)
    assert (int(out[0]["count"]), int(out[0]["frame_len"]), int(out[0]["last_len"])) == (1, 1020, 1020)
    assert arena[2:2 + 1020].tobytes() == F.emit_whole(d, F.DEFAULT)
    # cap one byte short / a stride below the frame length: sizes reported, nothing stored
    for kw in (dict(cap=572 + 468 - 1), dict(stride=571), dict(stride=600, cap=600 + 468 - 1)):
        out, arena = one(d, **kw)
        assert (int(out[0]["count"]), int(out[0]["frame_len"]), int(out[0]["last_len"]), int(out[0]["written"])) == (2, 572, 468, 0)
        assert (arena == C.SENTINEL).all()
    out, arena = one(d, stride=600, cap=600 + 468)
    assert out[0]["written"] == 1 and (arena[2 + 572:2 + 600] == C.SENTINEL).all() and arena[2 + 600] == 0x45
    # records that are not cut: the status is emit's, nothing else
    v6 = P.ipv6(bytes(16), bytes(16), 17, P.udp(7, 9, bytes(40)))
    for rec, kind in ((v6, E.KIND_IP), (P.eth(d, 0x0806), E.KIND_ETH), (d, E.KIND_RAW),
                      (P.ipv4(F.A, F.B, 17, P.udp(7, 9, bytes(40)), ihl=6), E.KIND_IP),
                      (P.ipv4(F.A, F.B, 17, P.udp(7, 9, bytes(40)), flags_frag=0x2000), E.KIND_IP),
                      (P.ipv4(F.A, F.B, 17, P.udp(7, 9, bytes(40)), flags_frag=0x0001), E.KIND_IP),
                      (d[:-1], E.KIND_IP)):
        out, arena = one(rec, kind)
        st = C.emit_record(rec, kind, 0, F.DEFAULT)[0]
        assert (int(out[0]["count"]), int(out[0]["written"]), int(out[0]["status"])) == (0, 0, st) and (arena == C.SENTINEL).all()
    out, arena = one(d, mtu=27)
    assert int(out[0]["count"]) == 0 and int(out[0]["status"]) == 0 and (arena == C.SENTINEL).all()
    # without caps.ipv4.tx() the fragment headers' checksums stay 0; without udp.tx() the L4 field is 0
    out, arena = one(d, caps=(1, 1, 0, 0, 0))
    assert arena[2 + 10:2 + 12].tobytes() == b"\0\0" and arena[2 + 26:2 + 28].tobytes() == b"\0\0" and out[0]["written"] == 1
    # a raw socket's datagram: cut, payload verbatim, status UNSUPPORTED
    out, arena = one(d, flags=E.REC_IPHDR_ONLY)
    assert out[0]["written"] == 1 and out[0]["status"] == F.ST_UNSUPPORTED and arena[2 + 20:2 + 572].tobytes() == d[20:572]
