"""CPU-side checks of tcp_segment_emit (smol_csum_batch_tcp_segment_emit): the symbol, the plan and result
structs in their three spellings (header, ctypes, numpy), the argument errors that need no device, and
tests/tcp_segment_ref.py, the numpy restatement of the cut that the GPU tests (tests/test_gpu_tcp_segment.py)
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
from tests import pktgen as P
from tests import tcp_segment_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "smol_csum_batch_tcp_segment_emit"
DEFAULT = (0, 0, 0, 0, 0)
ST_ACCEPT = 0x80


def _header_text():
    with open(os.path.join(ROOT, "include", "smolcsum.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_symbol_declared_exported_and_listed():
    text = _header_text()
    L = smoltcp_amd.lib()
    assert re.search(r"\b%s\s*\(" % NAME, text)
    assert hasattr(L, NAME) and NAME in _lib.ABI_SYMBOLS
    assert "smol_csum_tcpplan_t" in text and "smol_csum_tcpout_t" in text
    assert L.smol_csum_abi_version() == 6  # additive: the version stays


def _header_struct(name):
    body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % name, _header_text()).group(1)
    return [(t, n) for t, n in re.findall(r"(uint\d+_t)\s+(\w+);", body)]


def test_structs_are_32_and_16_bytes_in_every_spelling():
    size = {"uint8_t": 1, "uint16_t": 2, "uint32_t": 4, "uint64_t": 8}
    for cname, nbytes, cstruct, dts in (("smol_csum_tcpplan_t", 32, _lib.TcpPlanC, (E.TCPPLAN_DTYPE, T.TCPPLAN_DTYPE)),
                                        ("smol_csum_tcpout_t", 16, _lib.TcpOutC, (E.TCPOUT_DTYPE, T.TCPOUT_DTYPE))):
        fields = _header_struct(cname)
        assert sum(size[t] for t, _ in fields) == nbytes == ctypes.sizeof(cstruct)
        assert [n for _, n in fields] == [n for n, _ in cstruct._fields_] == list(dts[0].names)
        assert [size[t] for t, _ in fields] == [ctypes.sizeof(t) for _, t in cstruct._fields_]
        assert dts[0] == dts[1] and dts[0].itemsize == nbytes
    # the result entry is smol_csum_fragout_t's layout under its own name
    assert _header_struct("smol_csum_tcpout_t") == _header_struct("smol_csum_fragout_t")
    p = _lib.TcpPlanC(0x0807060504030201, 0x0C0B0A09, 0x0E0D, 0x100F, 0x1817161514131211, 0x1C1B1A19, 0x201F1E1D)
    assert list(bytes(p)) == list(range(1, 33))
    a = np.frombuffer(bytes(p), dtype=E.TCPPLAN_DTYPE)[0]
    assert [int(a[f]) for f in E.TCPPLAN_DTYPE.names] == \
        [0x0807060504030201, 0x0C0B0A09, 0x0E0D, 0x100F, 0x1817161514131211, 0x1C1B1A19, 0x201F1E1D]
    o = _lib.TcpOutC(0x04030201, 0x08070605, 0x0C0B0A09, 13, 14, 0x100F)
    assert list(bytes(o)) == list(range(1, 17))
    a = np.frombuffer(bytes(o), dtype=E.TCPOUT_DTYPE)[0]
    assert [int(a[f]) for f in E.TCPOUT_DTYPE.names] == [0x04030201, 0x08070605, 0x0C0B0A09, 13, 14, 0x100F]
    m = E.make_tcpplans([5, 9], [1000, 2000], 536, [7, 8], [100, 200])
    assert m.dtype == E.TCPPLAN_DTYPE and m["mss"].tolist() == [536, 536] and m["len"].tolist() == [1000, 2000]
    assert m["src_offset"].tolist() == [5, 9] and m["dst_offset"].tolist() == [7, 8] and m["cap"].tolist() == [100, 200]
    assert m["reserved"].tolist() == [0, 0] and m["reserved2"].tolist() == [0, 0]


def test_argument_errors_need_no_device():
    L = smoltcp_amd.lib()
    b = _lib.BatchC()
    b.n, b.stride, b.len, b.kind = 4, 64, 64, 1
    caps = _lib.Caps()
    buf = (ctypes.c_uint8 * 256)()
    src = (ctypes.c_uint8 * 64)()
    dst = (ctypes.c_uint8 * 64)()
    raw = (ctypes.c_uint8 * 224)()
    al = (ctypes.addressof(raw) + 15) & ~15  # 16-byte aligned: plans at al, out at al + 128
    pl, out = al, al + 128
    ctx = ctypes.c_void_p(1)  # never dereferenced: every case below fails its argument checks first
    call = getattr(L, NAME)
    B, Cp = ctypes.byref(b), ctypes.byref(caps)
    EINVAL = _lib.SMOL_EINVAL
    assert call(None, buf, B, Cp, src, dst, pl, 0, out, None) == EINVAL  # NULL ctx
    b.n = 0
    assert call(None, buf, B, Cp, src, dst, pl, 0, out, None) == EINVAL  # NULL ctx, also with nothing to do
    b.n = 4
    assert call(ctx, buf, B, None, src, dst, pl, 0, out, None) == EINVAL  # NULL caps
    assert call(ctx, None, B, Cp, src, dst, pl, 0, out, None) == EINVAL  # NULL d_buf
    assert call(ctx, buf, B, Cp, None, dst, pl, 0, out, None) == EINVAL  # NULL d_src
    assert call(ctx, buf, B, Cp, src, None, pl, 0, out, None) == EINVAL  # NULL d_dst
    assert call(ctx, buf, B, Cp, src, dst, None, 0, out, None) == EINVAL  # NULL d_plans
    assert call(ctx, buf, B, Cp, src, dst, pl, 0, None, None) == EINVAL  # NULL d_out
    assert call(ctx, buf, B, Cp, src, dst, pl + 8, 0, out, None) == EINVAL  # d_plans not 16-byte aligned
    assert call(ctx, buf, B, Cp, src, dst, pl, 0, out + 4, None) == EINVAL  # d_out not 16-byte aligned
    bad = _lib.Caps()
    bad.tcp = 4
    assert call(ctx, buf, B, ctypes.byref(bad), src, dst, pl, 0, out, None) == EINVAL  # bad caps value
    b.len = (1 << 30) + 1  # past SMOL_MAX_RECORD_LEN, as emit
    assert call(ctx, buf, B, Cp, src, dst, pl, 0, out, None) == _lib.SMOL_ERANGE
    assert L.smol_csum_batch_emit(ctx, buf, B, Cp, None, None) == _lib.SMOL_ERANGE
    b.len, b.n = 64, 0  # no records: OK whatever the arrays are, nothing launched
    assert call(ctx, None, B, Cp, None, None, None, 0, None, None) == _lib.SMOL_OK


def _one(rec, payload, mss, kind=E.KIND_IP, cap=1 << 20, stride=0, flags=0, caps=DEFAULT, at=2, arena=4000):
    src = np.frombuffer(b"\xee" * 3 + payload + b"\xee", np.uint8)
    plans = E.make_tcpplans([3], len(payload), mss, [at], cap)
    return T.expected([rec], [kind], [flags], plans, src, stride, caps, arena)


@pytest.mark.parametrize("v6,eth,doff", [(False, False, 5), (True, True, 8), (False, True, 15), (True, False, 5)])
def test_helper_cut_rules(v6, eth, doff):
    rng = np.random.default_rng(3 + doff)
    kind = E.KIND_ETH if eth else E.KIND_IP
    io, ihl, thl = (14 if eth else 0), (40 if v6 else 20), 4 * doff
    hl, t = io + ihl + thl, io + ihl
    seq0 = 0x11223344
    rec = T.template(rng, v6=v6, eth=eth, doff=doff, flags=0x18, seq=seq0, tail=b"ignored")
    pay = P.rand_bytes(rng, 1000)
    out, arena = _one(rec, pay, 536, kind)
    assert [int(out[0][f]) for f in ("count", "frame_len", "last_len", "written", "status")] == [2, hl + 536, hl + 464, 1, 0]
    f0, f1 = arena[2:2 + hl + 536].tobytes(), arena[2 + hl + 536:2 + 2 * hl + 1000].tobytes()
    assert (arena[:2] == T.SENTINEL).all() and (arena[2 + 2 * hl + 1000:] == T.SENTINEL).all()
    assert f0[hl:] == pay[:536] and f1[hl:] == pay[536:]
    assert int.from_bytes(f0[t + 4:t + 8], "big") == seq0 and int.from_bytes(f1[t + 4:t + 8], "big") == seq0 + 536
    assert f0[t + 13] == 0x10 and f1[t + 13] == 0x18  # PSH only on the last frame
    if v6:
        assert [int.from_bytes(f[io + 4:io + 6], "big") for f in (f0, f1)] == [thl + 536, thl + 464]
    else:
        assert [int.from_bytes(f[io + 2:io + 4], "big") for f in (f0, f1)] == [20 + thl + 536, 20 + thl + 464]
        assert f0[io + 4:io + 8] == f1[io + 4:io + 8] == rec[io + 4:io + 8] == b"\0\0\x40\0"  # ident 0, DF: every frame
    # everything else in the head is the template's, on both frames
    same = [i for i in range(hl) if i not in (t + 4, t + 5, t + 6, t + 7, t + 13, t + 16, t + 17) and
            i - io not in ((4, 5) if v6 else (2, 3, 10, 11))]
    assert all(f0[i] == f1[i] == rec[i] for i in same)
    # len 0: one frame, the emitted template
    out, arena = _one(rec, b"", 536, kind)
    assert [int(out[0][f]) for f in ("count", "frame_len", "last_len", "written")] == [1, hl, hl, 1]
    assert arena[2:2 + hl].tobytes() == T.emit_record(rec[:hl], kind, 0, DEFAULT)[1] and (arena[2 + hl:] == T.SENTINEL).all()
    # cap one byte short / a stride below the frame length: sizes reported, nothing stored
    for kw in (dict(cap=2 * hl + 1000 - 1), dict(stride=hl + 535), dict(stride=hl + 600, cap=2 * hl + 600 + 464 - 1)):
        out, arena = _one(rec, pay, 536, kind, **kw)
        assert [int(out[0][f]) for f in ("count", "frame_len", "last_len", "written")] == [2, hl + 536, hl + 464, 0]
        assert (arena == T.SENTINEL).all()
    out, arena = _one(rec, pay, 536, kind, stride=hl + 600, cap=2 * hl + 600 + 464)
    assert out[0]["written"] == 1 and (arena[2 + hl + 536:2 + hl + 600] == T.SENTINEL).all()
    assert arena[2 + hl + 600:2 + hl + 600 + hl + 464].tobytes() == f1
    # without caps.ipv4.tx() / caps.tcp.tx() the fields are 0
    out, arena = _one(rec, pay, 536, kind, caps=(1, 0, 3, 0, 0))
    assert arena[2 + t + 16:2 + t + 18].tobytes() == b"\0\0" and out[0]["written"] == 1
    if not v6:
        assert arena[2 + io + 10:2 + io + 12].tobytes() == b"\0\0"


def test_helper_flags_and_sequence_wrap():
    rng = np.random.default_rng(5)
    pay = P.rand_bytes(rng, 1000)
    for fl, ns in ((0x10, False), (0x18, False), (0x19, False), (0xF9, True)):
        rec = T.template(rng, flags=fl, ns=ns, seq=0xFFFFFF00)
        out, arena = _one(rec, pay, 100)
        assert int(out[0]["count"]) == 10 and out[0]["written"] == 1
        for k in range(10):
            f = arena[2 + 140 * k:2 + 140 * (k + 1)].tobytes()
            assert int.from_bytes(f[24:28], "big") == (0xFFFFFF00 + 100 * k) & 0xFFFFFFFF
            assert f[33] == (fl if k == 9 else fl & ~0x09) and f[32] == (0x51 if ns else 0x50)


def test_helper_records_not_cut():
    rng = np.random.default_rng(6)
    for name, rec, kind, flags, mss, ln in T.not_cut_cases(rng):
        src = np.zeros(ln + 3, np.uint8)
        plans = E.make_tcpplans([3], ln, mss, [2], 1 << 30)
        out, arena = T.expected([rec], [kind], [flags], plans, src, 0, DEFAULT, 64)
        st = T.emit_record(rec, kind, flags, DEFAULT)[0]
        assert (int(out[0]["count"]), int(out[0]["written"]), int(out[0]["status"])) == (0, 0, st), name
        assert int(out[0]["frame_len"]) == 0 and int(out[0]["last_len"]) == 0 and (arena == T.SENTINEL).all(), name


@pytest.mark.parametrize("v6", [False, True])
def test_helper_frames_pass_the_oracles_own_gate(v6):
    """Every frame the helper makes is accepted by oracle.batch_verify under default caps."""
    rng = np.random.default_rng(7 + v6)
    frames, kinds = [], []
    for eth in (False, True):
        for doff in (5, 8, 15):
            for mss, ln in ((1, 5), (7, 38), (536, 1000), (1460, 4380), (1460, 0)):
                kind = E.KIND_ETH if eth else E.KIND_IP
                rec = T.template(rng, v6=v6, eth=eth, doff=doff, flags=0x19)
                assert int.from_bytes(rec[-4 * doff:][0:2], "big") and int.from_bytes(rec[-4 * doff:][2:4], "big")  # ports non-zero
                st, fr = T.frames_of(rec, kind, 0, P.rand_bytes(rng, ln), mss, DEFAULT)
                assert st == 0 and len(fr) == max(1, -(-ln // mss))
                frames += fr
                kinds += [kind] * len(fr)
    buf, offs, lens = P.pack(frames, gap_rng=rng)
    st = P.oracle_verify_records(buf, offs, lens, np.array(kinds, np.uint8))
    assert ((st & ST_ACCEPT) != 0).all()
