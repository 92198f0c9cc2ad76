"""CPU-side checks of verify_tcp_assemble (smol_csum_batch_verify_tcp_assemble): the symbol, the window,
segment and flow structs in their spellings (header, ctypes, both numpy ones), the argument errors that need
no device, and tests/tcp_assemble_ref.py, the numpy restatement of the contract that the GPU tests
(tests/test_gpu_tcp_assemble.py) take their expected entries and ring bytes from: the window rule branch by
branch, the ring split, the equality with the reference's one-segment-at-a-time path and the differences
from it that the header states.  No kernel is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest

import smoltcp_amd
from smoltcp_amd import _lib
from smoltcp_amd import engine as E
from tests import pktgen as P
from tests import tcp_assemble_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "smol_csum_batch_verify_tcp_assemble"
A4, B4 = bytes([10, 1, 2, 3]), bytes([10, 4, 5, 6])


def _header_text():
    with open(os.path.join(ROOT, "include", "smolcsum.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_symbol_declared_exported_and_listed():
    text = _header_text()
    L = smoltcp_amd.lib()
    assert re.search(r"\b%s\s*\(" % NAME, text)
    assert hasattr(L, NAME) and NAME in _lib.ABI_SYMBOLS
    for t in ("smol_csum_tcpwin_t", "smol_csum_tcpseg_t", "smol_csum_tcpflow_t"):
        assert t in text
    assert re.search(r"#define\s+SMOL_MAX_FLOW_SEGMENTS\s+256u", text)
    assert E.MAX_FLOW_SEGMENTS == R.MAX_FLOW_SEGMENTS == 256
    for name, val in (("TCP", 1), ("IN_WINDOW", 2), ("COPIED", 4), ("REDELIVERED", 8)):
        assert int(re.search(r"#define\s+SMOL_SEG_%s\s+0x([0-9a-f]+)u" % name, text).group(1), 16) == val
        assert getattr(E, "SEG_" + name) == getattr(R, "SEG_" + name) == val
    assert L.smol_csum_abi_version() == 6  # additive: the version stays


def _header_struct(name):
    """[(bytes per element, field name, elements)] of a typedef struct in the header."""
    body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % name, _header_text()).group(1)
    return [(int(t) // 8, n, int(k or 1)) for t, n, k in re.findall(r"uint(\d+)_t\s+(\w+)(?:\[(\d+)\])?;", body)]


def test_structs_in_every_spelling():
    for cname, nbytes, cstruct, dts in (("smol_csum_tcpwin_t", 32, _lib.TcpWinC, (E.TCPWIN_DTYPE, R.TCPWIN_DTYPE)),
                                        ("smol_csum_tcpseg_t", 16, _lib.TcpSegC, (E.TCPSEG_DTYPE, R.TCPSEG_DTYPE)),
                                        ("smol_csum_tcpflow_t", 16, _lib.TcpFlowC, (E.TCPFLOW_DTYPE, R.TCPFLOW_DTYPE))):
        fields = _header_struct(cname)
        assert sum(sz * k for sz, _, k in fields) == nbytes == ctypes.sizeof(cstruct) == dts[0].itemsize
        assert [n for _, n, _ in fields] == [n for n, _ in cstruct._fields_] == list(dts[0].names)
        assert [sz * k for sz, _, k in fields] == [ctypes.sizeof(t) for _, t in cstruct._fields_] \
            == [dts[0].fields[n][0].itemsize for n in dts[0].names]
        assert dts[0] == dts[1]
    w = _lib.TcpWinC(0x0807060504030201, 0x0C0B0A09, 0x100F0E0D, 0x14131211, 0x18171615,
                     (ctypes.c_uint32 * 2)(0x1C1B1A19, 0x201F1E1D))
    assert list(bytes(w)) == list(range(1, 33))
    a = np.frombuffer(bytes(w), dtype=E.TCPWIN_DTYPE)[0]
    assert [int(a[f]) for f in E.TCPWIN_DTYPE.names[:5]] == [0x0807060504030201, 0x0C0B0A09, 0x100F0E0D, 0x14131211, 0x18171615]
    assert a["reserved"].tolist() == [0x1C1B1A19, 0x201F1E1D]
    s = _lib.TcpSegC(0x04030201, 0x08070605, 0x0C0B0A09, 0x0E0D, 15, 16)
    assert list(bytes(s)) == list(range(1, 17))
    a = np.frombuffer(bytes(s), dtype=E.TCPSEG_DTYPE)[0]
    assert [int(a[f]) for f in E.TCPSEG_DTYPE.names] == [0x04030201, 0x08070605, 0x0C0B0A09, 0x0E0D, 15, 16]
    f = _lib.TcpFlowC(0x04030201, 0x08070605, 0x0C0B0A09, 13, (ctypes.c_uint8 * 3)(14, 15, 16))
    assert list(bytes(f)) == list(range(1, 17))
    a = np.frombuffer(bytes(f), dtype=E.TCPFLOW_DTYPE)[0]
    assert [int(a[n]) for n in E.TCPFLOW_DTYPE.names[:4]] == [0x04030201, 0x08070605, 0x0C0B0A09, 13]
    assert a["reserved"].tolist() == [14, 15, 16]
    m = E.make_tcpwins([5, 1 << 33], [100, 200], 7, [0xFFFFFFFF, 3], 64)
    assert m.dtype == E.TCPWIN_DTYPE and m["dst_offset"].tolist() == [5, 1 << 33] and m["ring_len"].tolist() == [100, 200]
    assert m["ring_pos"].tolist() == [7, 7] and m["window_start"].tolist() == [0xFFFFFFFF, 3]
    assert m["window_len"].tolist() == [64, 64] and not m["reserved"].any()


def test_argument_errors_need_no_device():
    L = smoltcp_amd.lib()
    b = _lib.BatchC()
    b.n, b.stride, b.len, b.kind = 4, 64, 64, 1
    caps = _lib.Caps()
    buf = (ctypes.c_uint8 * 256)()
    dst = (ctypes.c_uint8 * 64)()
    st = (ctypes.c_uint8 * 8)()
    raw = (ctypes.c_uint8 * 160)()
    al = (ctypes.addressof(raw) + 15) & ~15  # 16-byte aligned: groups, wins (32 B), segs (4 x 16 B), flows
    g, w, sg, fl = al, al + 16, al + 48, al + 112
    ctx = ctypes.c_void_p(1)  # never dereferenced: every case below fails its argument checks first
    call = getattr(L, NAME)
    B, C = ctypes.byref(b), ctypes.byref(caps)
    EINVAL = _lib.SMOL_EINVAL
    assert call(None, buf, B, g, 1, C, dst, w, st, sg, fl, None) == EINVAL  # NULL ctx
    assert call(None, buf, B, g, 0, C, dst, w, st, sg, fl, None) == EINVAL  # NULL ctx, also with nothing to do
    assert call(ctx, buf, B, g, 1, None, dst, w, st, sg, fl, None) == EINVAL  # NULL caps
    assert call(ctx, buf, B, None, 1, C, dst, w, st, sg, fl, None) == EINVAL  # NULL d_groups
    assert call(ctx, buf, B, g, 1, C, None, w, st, sg, fl, None) == EINVAL  # NULL d_dst
    assert call(ctx, buf, B, g, 1, C, dst, None, st, sg, fl, None) == EINVAL  # NULL d_wins
    assert call(ctx, buf, B, g, 1, C, dst, w, None, sg, fl, None) == EINVAL  # NULL d_status
    assert call(ctx, buf, B, g, 1, C, dst, w, st, None, fl, None) == EINVAL  # NULL d_segs
    assert call(ctx, buf, B, g, 1, C, dst, w, st, sg, None, None) == EINVAL  # NULL d_flows
    assert call(ctx, buf, B, g + 8, 1, C, dst, w, st, sg, fl, None) == EINVAL  # d_groups not 16-byte aligned
    assert call(ctx, buf, B, g, 1, C, dst, w + 8, st, sg, fl, None) == EINVAL  # d_wins not 16-byte aligned
    assert call(ctx, buf, B, g, 1, C, dst, w, st, sg + 4, fl, None) == EINVAL  # d_segs not 16-byte aligned
    assert call(ctx, buf, B, g, 1, C, dst, w, st, sg, fl + 8, None) == EINVAL  # d_flows not 16-byte aligned
    bad = _lib.Caps()
    bad.tcp = 4
    assert call(ctx, buf, B, g, 1, ctypes.byref(bad), dst, w, st, sg, fl, None) == EINVAL  # bad caps value
    b.len = (1 << 30) + 1  # past SMOL_MAX_RECORD_LEN, as verify
    assert call(ctx, buf, B, g, 1, C, dst, w, st, sg, fl, None) == _lib.SMOL_ERANGE
    assert L.smol_csum_batch_verify(ctx, buf, B, C, st, None) == _lib.SMOL_ERANGE
    b.len = 64  # no groups: OK whatever the arrays are, nothing launched
    assert call(ctx, buf, B, None, 0, C, None, None, None, None, None, None) == _lib.SMOL_OK


# ---- the window rule ----

W0 = 1000  # window_start of the table


@pytest.mark.parametrize("s,p,W,want", [
    # (in_window, win_off, len, trim)
    (0, 10, 64, (1, 0, 10, 0)),       # in order
    (5, 10, 64, (1, 5, 10, 0)),       # out of order, inside
    (-4, 10, 64, (1, 0, 6, 4)),       # the front trimmed: the end is in the window
    (60, 10, 64, (1, 60, 4, 0)),      # the back trimmed: the start is in the window
    (54, 10, 64, (1, 54, 10, 0)),     # an end exactly at W
    (-10, 10, 64, (0, 0, 0, 0)),      # ends exactly at window_start: 0 < s + p fails
    (-9, 10, 64, (1, 0, 1, 9)),       # one byte inside
    (64, 10, 64, (0, 0, 0, 0)),       # starts at window_end
    (63, 10, 64, (1, 63, 1, 0)),      # last window byte
    (-3, 70, 64, (0, 0, 0, 0)),       # straddles the whole window: the reference's rule, not in the window
    (0, 70, 64, (1, 0, 64, 0)),       # starts at window_start and ends past window_end: the start rule
    (-3, 67, 64, (1, 0, 64, 3)),      # starts before, ends exactly at window_end: the end rule
    (0, 10, 0, (0, 0, 0, 0)),         # data against a closed window
    (-1, 0, 64, (0, 0, 0, 0)),        # keep-alive / window probe
    (-1, 0, 0, (0, 0, 0, 0)),         # the same against a closed window
    (0, 0, 0, (1, 0, 0, 0)),          # an empty segment in an empty window
    (1, 0, 0, (0, 0, 0, 0)),
    (0, 0, 64, (1, 0, 0, 0)),         # a bare ACK at window_start
    (63, 0, 64, (1, 63, 0, 0)),
    (64, 0, 64, (0, 0, 0, 0)),        # p = 0 at s = W
    (-2, 0, 64, (0, 0, 0, 0)),
    (-1, 1, 64, (0, 0, 0, 0)),        # a one-byte keep-alive with data: ends at window_start
])
def test_window_rule_table(s, p, W, want):
    for ws in (W0, 0, 0xFFFFFFFF, 0x80000000, 0x7FFFFFFF, 3, 0xFFFFFFF0):  # seq and window_start wrap around 2^32
        got = tuple(int(x) for x in R.window_rule((ws + s) & 0xFFFFFFFF, p, ws, W))
        assert got == want, (ws, got)


def _item(seq, payload, syn_rst=False, accept=True, off=54):
    return (seq & 0xFFFFFFFF, payload, off, syn_rst, accept)


def _win(window_start, window_len, ring_len=None, ring_pos=0, dst_offset=0):
    return E.make_tcpwins([dst_offset], ring_len if ring_len is not None else window_len, ring_pos, window_start, window_len)[0]


def test_syn_and_rst_report_the_window_and_are_never_copied():
    arena = np.full(80, R.SENTINEL, np.uint8)
    segs, flow = R.assemble_group([_item(W0 + 5, b"abcdef", syn_rst=True), _item(W0 + 70, b"x", syn_rst=True)], _win(W0, 64), arena)
    assert (int(segs[0]["win_off"]), int(segs[0]["len"]), int(segs[0]["flags"])) == (5, 6, R.SEG_TCP | R.SEG_IN_WINDOW)
    assert (int(segs[1]["win_off"]), int(segs[1]["len"]), int(segs[1]["flags"])) == (0, 0, R.SEG_TCP)
    assert (arena == R.SENTINEL).all() and int(flow["contig_len"]) == 0 and int(flow["counted"]) == 0 and flow["valid"] == 1


def test_ring_split_at_every_position_of_a_100_byte_ring():
    data = bytes(range(1, 61))
    for pos in range(100):
        for wo, ln in ((0, 60), (13, 47), (40, 1), (0, 100 - pos), (5, 0)):
            pos0, len0, len1 = (int(x) for x in R.ring_split(wo, ln, pos, 100))
            if ln == 0:
                assert (pos0, len0, len1) == (0, 0, 0)
                continue
            assert pos0 == (pos + wo) % 100 and len0 + len1 == ln and len0 > 0 and pos0 + len0 <= 100
            assert len1 == 0 or pos0 + len0 == 100
            if (wo, ln) == (0, 100 - pos):  # a piece ending exactly at the ring's end does not wrap
                assert (pos0, len0, len1) == (pos, 100 - pos, 0)
    # through assemble_group: the bytes land where write_unallocated puts them
    for pos in range(100):
        arena = np.full(107, R.SENTINEL, np.uint8)
        R.assemble_group([_item(W0 + 13, data[:47])], _win(W0, 60, ring_len=100, ring_pos=pos, dst_offset=3), arena)
        want = np.full(107, R.SENTINEL, np.uint8)
        want[3 + (pos + 13 + np.arange(47)) % 100] = np.frombuffer(data[:47], np.uint8)
        assert np.array_equal(arena, want), pos


# ---- against the reference's one-segment-at-a-time path ----

def _batch(segments, ws, W, ring_len, ring_pos, accept=None):
    arena = np.full(ring_len, R.SENTINEL, np.uint8)
    items = [_item(seq, pl, accept=True if accept is None else accept[i]) for i, (seq, pl) in enumerate(segments)]
    segs, flow = R.assemble_group(items, _win(ws, W, ring_len=ring_len, ring_pos=ring_pos), arena)
    return segs, flow, arena


def _front(ring, ring_pos, n):
    return ring[(ring_pos + np.arange(n)) % len(ring)]


@pytest.mark.parametrize("seed", range(40))
def test_equals_the_sequential_socket_when_overlaps_agree(seed):
    """Random flows whose payloads are slices of one byte stream: in order, shuffled, duplicated, with
    holes, some starting before the window, all ending at or before window_end.  [0, contig_len) of the
    ring and contig_len equal the socket fed one segment at a time (unbounded assembler)."""
    rng = np.random.default_rng(seed)
    W = int(rng.integers(1, 400))
    ring_len = W + int(rng.integers(0, 50))
    ring_pos = int(rng.integers(0, ring_len))
    ws = int(rng.choice([5, 0xFFFFFF00, 0x7FFFFFC0, 0xFFFFFFFF, int(rng.integers(0, 1 << 32))]))
    before = 40
    stream = P.rand_bytes(rng, before + W)  # stream[before + o] is the byte at window offset o
    segments = []
    for _ in range(int(rng.integers(1, 30))):
        a = int(rng.integers(-before, W))
        b = int(rng.integers(a, min(W, a + 80) + 1))
        segments.append(((ws + a) & 0xFFFFFFFF, stream[before + a:before + b]))
    mode = seed % 4
    if mode == 0:
        segments.sort(key=lambda t: int(R.seq_diff(t[0], ws)))
    elif mode == 1:
        segments += [segments[int(i)] for i in rng.integers(0, len(segments), 5)]
    elif mode == 2 and len(segments) > 3:  # holes: drop a few
        segments = [t for i, t in enumerate(segments) if i % 3]
    _, flow, arena = _batch(segments, ws, W, ring_len, ring_pos)
    seq = R.sequential_socket(segments, ws, W, ring_pos, ring_len)
    c = int(flow["contig_len"])
    assert c == seq["contig"]
    assert np.array_equal(_front(arena, ring_pos, c), _front(seq["ring"], ring_pos, c))
    assert _front(arena, ring_pos, c).tobytes() == stream[before:before + c]


def test_difference_a_duplicate_after_enqueue_is_reported_in_window():
    data = bytes(range(100, 140))
    segments = [(W0, data[:20]), (W0, data[:20])]
    segs, flow, _ = _batch(segments, W0, 64, 64, 0)
    seq = R.sequential_socket(segments, W0, 64, 0, 64)
    assert seq["in_window"] == [True, False]  # the window has moved past the duplicate
    assert all(int(f) & R.SEG_IN_WINDOW for f in segs["flags"])  # here it is tested against the poll's first window
    assert int(flow["contig_len"]) == seq["contig"] == 20 and int(flow["counted"]) == 2


def test_difference_a_straddle_past_window_end_after_an_advance():
    data = bytes(range(1, 101))
    segments = [(W0, data[:10]), (W0 + 5, data[5:80])]  # the second starts before the advanced window_start
    segs, flow, arena = _batch(segments, W0, 64, 64, 0)
    seq = R.sequential_socket(segments, W0, 64, 0, 64)
    assert seq["in_window"] == [True, False] and seq["contig"] == 10  # dropped by the reference
    assert (int(segs[1]["win_off"]), int(segs[1]["len"])) == (5, 59)  # trimmed and delivered here
    assert int(flow["contig_len"]) == 64 and arena.tobytes() == data[:64]


def test_difference_the_hole_limit():
    """Five isolated out-of-order segments, then the front: the reference's assembler (4 contigs) drops the
    fifth, this call computes the unbounded union."""
    data = P.rand_bytes(np.random.default_rng(1), 120)
    order = [100, 80, 60, 40, 20, 0]  # six holes' worth of arrivals, the front last
    segments = [(W0 + o, data[o:o + 10]) for o in order]
    fill = [(W0 + o + 10, data[o + 10:o + 20]) for o in order]
    _, flow, arena = _batch(segments + fill, W0, 120, 120, 0)
    assert int(flow["contig_len"]) == 120 and arena.tobytes() == data
    unbounded = R.sequential_socket(segments + fill, W0, 120, 0, 120)
    assert unbounded["contig"] == 120 and all(unbounded["stored"])
    four = R.sequential_socket(segments + fill, W0, 120, 0, 120, hole_limit=4)
    assert four["stored"][:6] == [True, True, True, True, False, True]  # the fifth island is dropped
    assert four["contig"] < 120


def test_corrupted_segment_and_its_retransmission():
    good = bytes(range(10, 54))
    bad = bytes(40)
    segments = [(W0 + 4, bad), (W0, good[:4]), (W0 + 4, good[4:44]), (W0 + 50, b"zz")]
    segs, flow, arena = _batch(segments, W0, 64, 64, 0, accept=[False, True, True, True])
    assert arena[:44].tobytes() == good[:4] + good[4:44] and arena[50:52].tobytes() == b"zz"
    assert [bool(int(f) & R.SEG_REDELIVERED) for f in segs["flags"]] == [False, False, True, False]
    assert (int(flow["contig_len"]), int(flow["counted"]), int(flow["redelivered"])) == (44, 3, 1)
    # the corrupted copy alone: its bytes lie in the ring, nothing counts
    segs, flow, arena = _batch(segments[:1], W0, 64, 64, 0, accept=[False])
    assert arena[4:44].tobytes() == bad and (int(flow["contig_len"]), int(flow["counted"])) == (0, 0)
    assert int(segs[0]["flags"]) == R.SEG_TCP | R.SEG_IN_WINDOW | R.SEG_COPIED


def test_expected_on_frames():
    """`expected` over real frames: Ethernet + IPv4 + TCP, a UDP record, a SYN, invalid groups."""
    rng = np.random.default_rng(2)
    data = P.rand_bytes(rng, 64)
    f = lambda seq, pl, flags=0x18, doff=5: P.eth(P.ipv4(A4, B4, 6, P.tcp(1000, 80, pl, seq=seq, flags=flags, doff=doff)))
    recs = [f(W0, data[:30]), f(W0 + 30, data[30:64], doff=8), P.eth(P.ipv4(A4, B4, 17, P.udp(7, 9, b"udp"))),
            f(W0 + 1, b"syn", flags=0x02), f(W0, data[:8])]
    n = len(recs)
    wins = E.make_tcpwins([2, 70, 70, 70], [64, 64, 64, 10], [60, 0, 0, 0], W0, [64, 64, 64, 11])
    wins["reserved"][2] = (0, 1)
    groups = [(0, 4, 0), (4, 1, 1), (4, 1, 0), (4, 1, 0)]  # reserved set; the window's reserved set; window_len > ring_len
    segs, flows, arena, written = R.expected(recs, [E.KIND_ETH] * n, [0] * n, groups, wins, [True] * n, 140)
    assert written.tolist() == [True, True, True, True, False]
    assert flows["valid"].tolist() == [1, 0, 0, 0] and int(flows[0]["contig_len"]) == 64 and int(flows[0]["counted"]) == 2
    assert segs["off"].tolist() == [54, 66, 0, 54, 0] and segs["seq"].tolist() == [W0, W0 + 30, 0, W0 + 1, 0]
    assert segs["flags"].tolist() == [7, 7, 0, 3, 0]
    assert arena[2 + (60 + np.arange(64)) % 64].tobytes() == data
    assert (arena[:2] == R.SENTINEL).all() and (arena[66:] == R.SENTINEL).all()
    # a window whose ring_pos is outside the ring, and one with ring_len 0 and ring_pos 0 (valid: nothing fits)
    w2 = E.make_tcpwins([0, 0], [64, 0], [64, 0], W0, [64, 0])
    _, flows, arena, written = R.expected(recs, [E.KIND_ETH] * n, [0] * n, [(0, 1, 0), (0, 1, 0)], w2, [True] * n, 64)
    assert flows["valid"].tolist() == [0, 1] and (arena == R.SENTINEL).all() and written.tolist() == [True] + [False] * 4
