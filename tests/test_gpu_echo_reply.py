"""GPU parity of verify_echo_reply (smol_csum_batch_verify_echo_reply): verify's status bytes, each record's
8-byte entry and the reply frames written into the records' slots of a second device buffer, in one pass.

Expected values in every case come from tests/echo_ref.py: the status bytes are the oracle's verify, the
REQUEST and address rules and the head bytes its own restatement of the header text, every reply checksum
the oracle's emit on the reply frame.  All comparisons are exact: status, entries, the WHOLE arena (filled
with the sentinel 0xA5, so a stray store anywhere fails), and the batch buffer unchanged.  Each test asserts
that the classes it means to exercise occur in its batch."""
import numpy as np
import pytest

import oracle
from tests import cut_ref as C
from tests import echo_ref as R
from tests import pktgen as P
from tests.test_echo_rule_cpu import BCAST, sweep

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from smoltcp_amd import engine as E  # noqa: E402

NOCAPS = (0, 0, 0, 0, 0)
V4A, V4B = bytes([10, 1, 2, 3]), bytes([10, 4, 5, 6])
V6A, V6B = bytes(range(0x20, 0x30)), bytes(range(0x40, 0x50))
MCAST4, MCAST6 = bytes([224, 0, 0, 1]), bytes.fromhex("ff02") + bytes(13) + b"\x01"
# the launch shapes of the kernel's shape set, by the number set_shape takes: (G, U)
SHAPES = {0: (8, 6), 7: (8, 7), 1: (16, 3), 8: (16, 4), 4: (32, 4), 6: (64, 4)}


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    e = E.ChecksumEngine(0)
    yield e
    e.close()


# ---- packets ---------------------------------------------------------------------------------------

def icmp(t: int, data: bytes, rng, code: int = 0) -> bytes:
    """An ICMP echo-shaped message: type, code, a zero checksum, random ident and sequence number, data."""
    return bytes([t, code, 0, 0]) + P.rand_bytes(rng, 4) + data


def echo4(rng, dlen: int, src=V4A, dst=V4B, ihl: int = 5) -> bytes:
    return P.ipv4(src, dst, 1, icmp(8, P.rand_bytes(rng, dlen), rng), ihl=ihl, options=bytes([1]) * (ihl * 4 - 20),
                  ident=int(rng.integers(0, 65536)), ttl=int(rng.integers(1, 256)))


def echo6(rng, dlen: int, src=V6A, dst=V6B, hbh_units=None) -> bytes:
    msg = icmp(128, P.rand_bytes(rng, dlen), rng)
    if hbh_units is None:
        return P.ipv6(src, dst, 58, msg, hop=int(rng.integers(1, 256)))
    return P.ipv6(src, dst, 0, P.hbh(58, hbh_units, rng) + msg)


def eth(r: bytes, mac_dst=None, mac_src=None) -> bytes:
    f = P.eth(r, 0x0800 if r[0] >> 4 == 4 else 0x86DD)
    return (mac_dst or f[0:6]) + (mac_src or f[6:12]) + f[12:]


def request(rng, ver: int, kind: int, dlen: int, **kw) -> bytes:
    r = echo4(rng, dlen, **kw) if ver == 4 else echo6(rng, dlen, **kw)
    return eth(r) if kind == E.KIND_ETH else r


# ---- one call, compared exactly ----------------------------------------------------------------------

def _prepare(recs, kinds, rflags=0, caps=NOCAPS, cfg=None, fixed=None, offs=None, flips=(), cap_adj=0, cap_abs=None,
             dst_mod=None, seed=0):
    """The batch buffer (every checksum filled by the oracle's emit, then `flips` = (record, byte, bit) corrupt
    single bits), slots back to back (dst_mod[i]: the slot's start at that residue mod 16, the gap showing the
    sentinel) with cap = the reply's length + cap_adj (cap_abs: that cap for all), and the reference's results."""
    n = len(recs)
    rng = np.random.default_rng(seed)
    kinds_a = np.broadcast_to(np.asarray(kinds, np.uint8), (n,)).copy()
    flags_a = np.broadcast_to(np.asarray(rflags, np.uint8), (n,)).copy()
    if offs is not None:
        end = max(int(o) + len(r) for o, r in zip(offs, recs))
        buf = rng.integers(0, 256, end + 16, dtype=np.uint8)
        for o, r in zip(offs, recs):
            buf[int(o):int(o) + len(r)] = np.frombuffer(r, np.uint8)
        offs, lens = np.asarray(offs, np.uint64), np.array([len(r) for r in recs], np.uint32)
    else:
        buf, offs, lens, _ = C.place_records(recs, kinds_a, flags_a, fixed, rng)
    oracle.batch_emit(buf, E.make_descriptors(offs, lens, kinds_a, flags_a), n)
    for i, o, bit in flips:
        buf[int(offs[i]) + o] ^= 1 << bit
    placed = [bytes(buf[int(o):int(o) + int(ln)]) for o, ln in zip(offs, lens)]
    need = R.frame_lens(placed, kinds_a, flags_a, cfg)
    cap = np.maximum(need + cap_adj, 0) if cap_abs is None else np.full(n, cap_abs, np.int64)
    d_offs, pos = np.zeros(n, np.uint64), 3
    for i in range(n):
        if dst_mod is not None:
            pos += (int(dst_mod[i]) - pos) % 16
        d_offs[i] = pos
        pos += int(cap[i])
    slots = E.make_slots(d_offs, cap)
    st, ent, arena = R.expected(placed, kinds_a, flags_a, caps, cfg, slots, pos + 21)
    return dict(buf=buf, offs=offs, lens=lens, kinds=kinds_a, flags=flags_a, fixed=fixed, caps=caps, cfg=cfg, slots=slots,
                status=st, entries=ent, arena=arena, fl=ent["flags"].astype(np.int64))


def _call(eng, b, shape=-1, blocks=0, stream=None):
    """The call on a prepared batch; every assertion of a case.  Returns the device arena."""
    eng.set_shape(shape)
    eng.set_max_blocks(blocks)
    try:
        batch, d, dv, dst, sd = C.upload(E, b["buf"], b["offs"], b["lens"], b["kinds"], b["flags"], b["fixed"], b["slots"],
                                         b["arena"].size)
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                st, ent = eng.verify_echo_reply(dv, batch, dst, sd, caps=b["caps"], cfg=b["cfg"], stream=stream)
            stream.synchronize()
        else:
            st, ent = eng.verify_echo_reply(dv, batch, dst, sd, caps=b["caps"], cfg=b["cfg"])
        launched = eng.last_launch()
        got_st, got_dst = st.cpu().numpy(), dst.cpu().numpy()
        got_ent = ent.cpu().numpy().reshape(-1).view(E.ECHO_DTYPE)
        assert np.array_equal(d.cpu().numpy(), b["buf"]), "the batch buffer is only read"
    finally:
        eng.set_shape(-1)
        eng.set_max_blocks(0)
    assert launched["kernel"] == "echo" and launched["variant"] == 0, launched
    if shape >= 0:
        assert (launched["G"], launched["U"]) == SHAPES[shape], launched
    bad = np.nonzero(got_st != b["status"])[0]
    assert bad.size == 0, f"status differs at {bad[:8]}: got {got_st[bad[:8]]} want {b['status'][bad[:8]]}"
    bad = np.nonzero(got_ent != b["entries"])[0]
    assert bad.size == 0, f"entries differ at {bad[:8]}: got {got_ent[bad[:4]]} want {b['entries'][bad[:4]]}"
    diff = np.nonzero(got_dst != b["arena"])[0]
    assert diff.size == 0, f"arena bytes differ at {diff[:8]} (got {got_dst[diff[:8]]} want {b['arena'][diff[:8]]})"
    return dst


def _run(eng, recs, kinds, shape=-1, blocks=0, stream=None, **kw):
    b = _prepare(recs, kinds, **kw)
    _call(eng, b, shape, blocks, stream)
    return b


def _has(b, flags: int, n: int = 1) -> bool:
    return int((b["fl"] == flags).sum()) >= n


FULL = R.REQUEST | R.ANSWERED | R.WRITTEN | R.SEND


# ---- data lengths at every alignment ----------------------------------------------------------------

# 111 / 112 / 113: Ethernet + IPv4 + ICMP heads end at byte 42, so the data ends around the window's edge at
# 128 + 26 and the 16-B grid's at 144 + 10; 8972 is a jumbo frame's
LENGTHS = (0, 1, 2, 3, 15, 16, 17, 31, 33, 56, 111, 112, 113, 1472, 8972)


@pytest.mark.parametrize("ver", [4, 6])
@pytest.mark.parametrize("kind", [E.KIND_IP, E.KIND_ETH])
def test_data_lengths_at_every_alignment(eng, ver, kind):
    """Every pair of (record start mod 16, slot start mod 16) at each data length: the head store, the shifted
    copy and both edge stores at every alignment, the slots next to each other."""
    rng = np.random.default_rng(10 * ver + kind)
    recs, offs, dmod, pos = [], [], [], 0
    for ln in LENGTHS:
        for sa in range(16):
            for da in range(16):
                r = request(rng, ver, kind, ln)
                pos += (sa - pos) % 16  # the device buffers are 16-byte aligned
                offs.append(pos)
                recs.append(r)
                dmod.append(da)
                pos += len(r)
    b = _run(eng, recs, kind, offs=np.array(offs, np.uint64), dst_mod=dmod, seed=ver)
    assert (b["fl"] == FULL).all() and len(recs) == len(LENGTHS) * 256
    hl = (14 if kind == E.KIND_ETH else 0) + (28 if ver == 4 else 48)
    assert (b["entries"]["head_len"] == hl).all()
    assert sorted(set((b["entries"]["frame_len"] - hl).tolist())) == sorted(LENGTHS)


def test_ipv4_options_and_hop_by_hop_headers_are_not_carried(eng):
    """IHL 6 and 15, a short Hop-by-Hop header and one longer than the 128-B window (ident and sequence number
    then come from global memory): the reply has a plain 20- / 40-byte IP header."""
    rng = np.random.default_rng(21)
    recs, kinds = [], []
    for i in range(240):
        ln = (0, 5, 56, 200, 77, 1300)[i % 6]
        kind = E.KIND_ETH if (i // 6) % 2 else E.KIND_IP
        m = (i // 12) % 4
        r = (echo4(rng, ln, ihl=6) if m == 0 else echo4(rng, ln, ihl=15) if m == 1 else
             echo6(rng, ln, hbh_units=0) if m == 2 else echo6(rng, ln, hbh_units=20))
        recs.append(eth(r) if kind == E.KIND_ETH else r)
        kinds.append(kind)
    b = _run(eng, recs, kinds, seed=22)
    assert (b["fl"] == FULL).all()
    e = np.where(np.array(kinds) == E.KIND_ETH, 14, 0)
    assert set((b["entries"]["head_len"] - e).tolist()) == {28, 48}
    assert int(b["entries"]["data_off"].max()) == 14 + 40 + 168 + 8  # behind the long Hop-by-Hop header


# ---- every launch shape -----------------------------------------------------------------------------

def _mixed_requests(rng, n, kind, maxlen):
    recs = []
    for i in range(n):
        ln = int(rng.integers(0, maxlen)) if i % 3 else int(rng.integers(0, 120))
        recs.append(request(rng, 4 if i % 2 else 6, kind, ln))
    return recs


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("fixed", [False, True])
def test_every_shape(eng, shape, fixed):
    """Each shape of the shape set forced through set_shape.  The fixed-stride batch's stride exceeds every
    datagram: the random bytes behind a datagram are neither summed nor echoed."""
    rng = np.random.default_rng(100 + shape)
    kind = E.KIND_ETH if shape % 2 else E.KIND_IP
    recs = _mixed_requests(rng, 300, kind, 1400 if fixed else 3000)
    flips = [(i, len(recs[i]) - 1 - int(rng.integers(0, 8)), int(rng.integers(0, 8))) for i in range(5, 300, 17)]
    b = _run(eng, recs, kind, shape=shape, fixed=(1531, 7) if fixed else None, flips=flips, seed=shape)
    assert _has(b, FULL, 200) and _has(b, FULL & ~R.SEND, 10)
    if fixed:
        assert (b["entries"]["frame_len"] < 1531 - 10).all()


@pytest.mark.parametrize("shape", [-1, 0, 6])
def test_ethernet_padding_is_not_echoed(eng, shape):
    """60-byte Ethernet frames at a fixed stride: one half carry an 18-byte-data request (the frame exactly),
    the other half a 5-byte-data one and 13 bytes of padding, which the reply must not carry."""
    rng = np.random.default_rng(31)
    recs = []
    for i in range(200):
        r = eth(echo4(rng, 18 if i % 2 else 5))
        recs.append(r + P.rand_bytes(rng, 60 - len(r)))
    b = _run(eng, recs, E.KIND_ETH, shape=shape, fixed=(60, 4), seed=32)
    assert (b["fl"] == FULL).all()
    assert sorted(set(b["entries"]["frame_len"].tolist())) == [47, 60]


# ---- caps -------------------------------------------------------------------------------------------

def _caps_batch(ver):
    rng = np.random.default_rng(40 + ver)
    recs, flips = [], []
    for i in range(120):
        kind_eth = i % 2 == 1
        dlen = int(rng.integers(0, 300))
        r = echo4(rng, dlen) if ver == 4 else echo6(rng, dlen)
        e = 14 if kind_eth else 0
        recs.append(eth(r) if kind_eth else r)
        if i % 4 == 1:  # the ICMP checksum, or the last data byte under it
            flips.append((i, e + (20 if ver == 4 else 40) + (2 if i % 8 == 1 or dlen == 0 else 7 + dlen), i % 8))
        elif i % 4 == 2 and ver == 4:  # the IPv4 header checksum
            flips.append((i, e + 10 + i % 2, i % 8))
    kinds = [E.KIND_ETH if i % 2 else E.KIND_IP for i in range(120)]
    return recs, kinds, flips


@pytest.mark.parametrize("ipv4", [0, 1, 2, 3])
@pytest.mark.parametrize("icmpv4", [0, 1, 2, 3])
def test_caps_ipv4(eng, ipv4, icmpv4):
    recs, kinds, flips = _caps_batch(4)
    b = _run(eng, recs, kinds, caps=(ipv4, 3, 3, icmpv4, 3), flips=flips, seed=41)
    assert (b["fl"] & R.WRITTEN).all()
    rx_any = ipv4 in (0, 1) or icmpv4 in (0, 1)
    assert _has(b, FULL & ~R.SEND, 20) == rx_any  # written, not to be sent: a gate that is on caught the request
    if not rx_any:
        assert (b["fl"] == FULL).all()  # accepted unchecked: the reply's checksums are the filled ones all the same
    # the reply's fields are zero exactly when tx is off
    for i in (0, 1):
        o, e = int(b["slots"][i]["dst_offset"]), 14 * i
        assert bool(b["arena"][o + e + 10:o + e + 12].any()) == (ipv4 in (0, 2))
        assert bool(b["arena"][o + e + 22:o + e + 24].any()) == (icmpv4 in (0, 2))


@pytest.mark.parametrize("icmpv6", [0, 1, 2, 3])
def test_caps_ipv6(eng, icmpv6):
    recs, kinds, flips = _caps_batch(6)
    b = _run(eng, recs, kinds, caps=(3, 3, 3, 3, icmpv6), flips=flips, seed=42)
    assert (b["fl"] & R.WRITTEN).all()
    assert _has(b, FULL & ~R.SEND, 20) == (icmpv6 in (0, 1))
    for i in (0, 1):
        o, e = int(b["slots"][i]["dst_offset"]), 14 * i
        assert bool(b["arena"][o + e + 42:o + e + 44].any()) == (icmpv6 in (0, 2))


# ---- the address rule -------------------------------------------------------------------------------

@pytest.mark.parametrize("with_cfg", [False, True])
def test_address_rule_table(eng, with_cfg):
    """One record per row of the rule's table (tests/test_echo_rule_cpu.py's sweep at one data length), with cfg
    NULL and with bcast_v4 set."""
    recs, kinds, want = [], [], []
    for kind, ver, md, ms, et, s, d, bc, ids, ln in sweep():
        if ln != 56 or (bc is not None) != with_cfg:
            continue
        msg = bytes([8 if ver == 4 else 128, 0, 0, 0]) + ids + bytes(range(56))
        r = P.ipv4(s, d, 1, msg) if ver == 4 else P.ipv6(s, d, 58, msg)
        recs.append(md + ms + et + r if kind == E.KIND_ETH else r)
        kinds.append(kind)
        want.append(R.rule(kind, ver, md, ms, s, d, bc))
    b = _run(eng, recs, kinds, cfg=BCAST if with_cfg else None, seed=51)
    assert ((b["fl"] & (R.REQUEST | R.ANSWERED | R.HOST)) == np.array(want)).all()
    assert _has(b, FULL, 30) and _has(b, R.REQUEST | R.HOST, 30) and _has(b, R.REQUEST, 30)
    assert len(recs) == 2 * (7 * 7 + 5 * 5) * 4


# ---- records that are no requests -------------------------------------------------------------------

def _non_requests(rng):
    """(record, kind, record flags) of everything that must leave an all-zero entry and an untouched slot."""
    pay = P.rand_bytes(rng, int(rng.integers(8, 200)))
    inner = P.ipv4(V4B, V4A, 17, P.udp(7, 9, pay[:8]))
    u4 = P.ipv4(V4A, V4B, 17, P.udp(7, 9, pay))
    rq4, rq6 = echo4(rng, len(pay)), echo6(rng, len(pay))
    out = [
        (P.ipv4(V4A, V4B, 1, icmp(0, pay, rng)), E.KIND_IP, 0),              # echo replies
        (P.ipv6(V6A, V6B, 58, icmp(129, pay, rng)), E.KIND_IP, 0),
        (P.ipv4(V4A, V4B, 1, icmp(8, pay, rng, code=1)), E.KIND_IP, 0),      # code != 0
        (P.ipv6(V6A, V6B, 58, icmp(128, pay, rng, code=7)), E.KIND_IP, 0),
        (P.ipv4(V4A, V4B, 1, P.icmp4_error(3, 1, inner)), E.KIND_IP, 0),     # ICMPv4 errors
        (P.ipv4(V4A, V4B, 1, P.icmp4_error(11, 0, inner)), E.KIND_IP, 0),
        (P.ipv6(V6A, V6B, 58, P.icmp6(135, 20 + 8, rng)), E.KIND_IP, 0),     # NDISC
        (P.ipv6(V6A, V6B, 58, P.icmp6(136, 20, rng)), E.KIND_IP, 0),
        (u4, E.KIND_IP, 0),
        (P.ipv6(V6A, V6B, 6, P.tcp(7, 9, pay)), E.KIND_IP, 0),
        (P.ipv4(V4A, V4B, 2, bytes([0x11, 0, 0, 0, 224, 0, 0, 1])), E.KIND_IP, 0),  # IGMP
        (P.ipv4(V4A, V4B, 1, rq4[20:], flags_frag=0x2000), E.KIND_IP, 0),    # fragments
        (P.ipv4(V4A, V4B, 1, rq4[20:], flags_frag=0x0003), E.KIND_IP, 0),
        (rq4, E.KIND_IP, E.REC_IPHDR_ONLY),
        (rq6, E.KIND_IP, E.REC_IPHDR_ONLY),
        (rq4, E.KIND_RAW, 0),
        (P.eth(rq4, 0x0806), E.KIND_ETH, 0),                                 # a non-IP ethertype
        (P.eth(rq4, 0x86DD), E.KIND_ETH, 0),                                 # ethertype / version mismatch
        (P.ipv6(V6A, V6B, 0, P.hbh_opts(58, bytes([0xC2, 0])) + rq6[40:]), E.KIND_IP, 0),  # Hop-by-Hop drop
    ]
    for l4 in (4, 5, 6, 7):  # truncated ICMP: an L4 buffer of 4 .. 7 bytes
        out.append((P.ipv4(V4A, V4B, 1, icmp(8, b"", rng)[:l4]), E.KIND_IP, 0))
        out.append((eth(P.ipv6(V6A, V6B, 58, icmp(128, b"", rng)[:l4])), E.KIND_ETH, 0))
    return out


def test_non_requests_between_requests(eng):
    rng = np.random.default_rng(61)
    recs, kinds, rflags, isreq = [], [], [], []
    for _ in range(12):
        for r, k, f in _non_requests(rng):
            recs.append(r), kinds.append(k), rflags.append(f), isreq.append(False)
            recs.append(request(rng, 4 if len(recs) % 4 else 6, E.KIND_ETH, int(rng.integers(0, 90))))
            kinds.append(E.KIND_ETH), rflags.append(0), isreq.append(True)
    b = _run(eng, recs, kinds, rflags=rflags, seed=62)
    isreq = np.array(isreq)
    assert (b["fl"][isreq] == FULL).all()
    assert not b["entries"][~isreq].view(np.uint8).any(), "a record that is no request has an entry"
    other = b["status"][~isreq]  # accepted with every gate passed, unsupported, malformed
    assert (other & (E.ST_MALFORMED | E.ST_UNSUPPORTED) == 0).any()
    assert (other & E.ST_MALFORMED).any() and (other & E.ST_UNSUPPORTED).any()


# ---- the cap ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["fit", "one_short", "zero"])
def test_cap(eng, mode):
    rng = np.random.default_rng(71)
    recs = _mixed_requests(rng, 240, E.KIND_ETH, 2000)
    b = _run(eng, recs, E.KIND_ETH, seed=72, **({"cap_adj": 0} if mode == "fit" else {"cap_adj": -1} if mode == "one_short"
                                              else {"cap_abs": 0}))
    if mode == "fit":
        assert (b["fl"] == FULL).all()
    else:  # answered, not written: the lengths reported, the arena untouched
        assert (b["fl"] == R.REQUEST | R.ANSWERED).all() and (b["arena"] == C.SENTINEL).all()
        assert (b["entries"]["frame_len"] >= 42).all() and (b["entries"]["head_len"] >= 42).all()


# ---- the grid stride, a side stream, the empty batch ---------------------------------------------------

def _mix(rng, n):
    """Mixed records of a descriptor batch: (records, kinds, record flags, flips, cap adjustment per record)."""
    recs, kinds, rflags, flips, adj = [], [], [], [], np.zeros(n, np.int64)
    others = []
    for i in range(n):
        c = int(rng.integers(0, 100))
        kind = E.KIND_ETH if rng.integers(0, 2) else E.KIND_IP
        ver = 4 if rng.integers(0, 2) else 6
        ln = int(rng.integers(0, 1500)) if rng.integers(0, 4) else int(rng.integers(0, 100))
        f = 0
        if c < 50:  # answered and sent
            r = request(rng, ver, kind, ln)
        elif c < 57:  # a corrupted request: written, not sent
            r = request(rng, ver, kind, ln)
            flips.append((i, len(r) - 1 - int(rng.integers(0, min(8, ln + 8))), int(rng.integers(0, 8))))
        elif c < 63:  # a slot too short
            r = request(rng, ver, kind, ln)
            adj[i] = -1 - int(rng.integers(0, 40))
        elif c < 70:  # the host's: a broadcast / multicast destination, a group MAC
            m = int(rng.integers(0, 3))
            if m == 0 or kind == E.KIND_IP:
                r = request(rng, ver, kind, ln, dst=bytes([255] * 4) if ver == 4 else MCAST6)
            else:
                r = echo4(rng, ln) if ver == 4 else echo6(rng, ln)
                r = eth(r, mac_dst=bytes([0xFF] * 6)) if m == 1 else eth(r, mac_src=bytes([0x03, 0, 0, 0, 0, 9]))
        elif c < 76:  # nobody answers: a multicast IPv4 destination, a non-unicast source
            m = int(rng.integers(0, 3))
            kw = {"dst": MCAST4} if m == 0 and ver == 4 else {"src": bytes(4) if ver == 4 else MCAST6}
            r = request(rng, ver, kind, ln, **kw)
        else:  # no request
            if not others:
                others = _non_requests(rng)
                rng.shuffle(others)
            r, kind, f = others.pop()
        recs.append(r), kinds.append(kind), rflags.append(f)
    return recs, kinds, rflags, flips, adj


def test_grid_stride_over_one_workgroup(eng):
    rng = np.random.default_rng(81)
    recs, kinds, rflags, flips, adj = _mix(rng, 1000)
    b = _run(eng, recs, kinds, rflags=rflags, flips=flips, cap_adj=adj, blocks=1, seed=82)
    assert _has(b, FULL, 300) and _has(b, 0, 100)


def test_side_stream_and_empty_batch(eng):
    rng = np.random.default_rng(91)
    recs, kinds, rflags, flips, adj = _mix(rng, 300)
    b = _run(eng, recs, kinds, rflags=rflags, flips=flips, cap_adj=adj, stream=torch.cuda.Stream(), seed=92)
    assert _has(b, FULL, 80)
    e = torch.zeros(64, dtype=torch.uint8, device="cuda")
    st, ent = eng.verify_echo_reply(e, E.Batch.fixed(0, 64, 64, E.KIND_IP), e, e)
    assert st.numel() == 0 and ent.numel() == 0


# ---- round trip -------------------------------------------------------------------------------------

def test_written_replies_verify(eng):
    """The written replies of a batch fed back as a descriptor batch: every one passes verify with rx on."""
    rng = np.random.default_rng(95)
    recs, kinds = [], []
    for i in range(400):
        kinds.append(E.KIND_ETH if i % 2 else E.KIND_IP)
        recs.append(request(rng, 4 if i % 4 < 2 else 6, kinds[-1], int(rng.integers(0, 1500)) if i % 5 else i % 7))
    b = _prepare(recs, kinds, seed=96)
    dst = _call(eng, b)
    w = (b["fl"] & R.WRITTEN) != 0
    assert w.all()
    back = E.Batch.from_records(b["slots"]["dst_offset"][w], b["entries"]["frame_len"][w], b["kinds"][w], "cuda:0")
    st = eng.verify(dst, back).cpu().numpy()
    assert (st & E.ST_ACCEPT).all() and (st & E.ST_IP_VALID).all() and (st & E.ST_L4_VALID).all()
    # and they are replies: fed to the call itself, none is a request
    slots = torch.zeros(16 * int(w.sum()), dtype=torch.uint8, device="cuda")
    _, ent = eng.verify_echo_reply(dst.clone(), back, dst, slots)
    assert not ent.cpu().numpy().any()


# ---- randomized mix ---------------------------------------------------------------------------------

def test_randomized_mix(eng):
    rng = np.random.default_rng(2024)
    recs, kinds, rflags, flips, adj = _mix(rng, 4096)
    b = _prepare(recs, kinds, rflags=rflags, flips=flips, cap_adj=adj, seed=2025)
    assert int((b["fl"] & R.SEND != 0).sum()) >= 1200, "the mix holds too few replies to send"
    for name, fl in (("written, not sent", FULL & ~R.SEND), ("answered, not written", R.REQUEST | R.ANSWERED),
                     ("the host's", R.REQUEST | R.HOST), ("a request nobody answers", R.REQUEST), ("no request", 0)):
        assert _has(b, fl, 20), f"the mix holds fewer than 20 records of class: {name}"
    assert set(b["fl"].tolist()) == {FULL, FULL & ~R.SEND, R.REQUEST | R.ANSWERED, R.REQUEST | R.HOST, R.REQUEST, 0}
    _call(eng, b)
