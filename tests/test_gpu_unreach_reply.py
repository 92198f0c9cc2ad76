"""GPU parity of verify_unreach_reply (smol_csum_batch_verify_unreach_reply): verify's status bytes, each
record's 8-byte entry and the ICMP error frames written into the records' slots of a second device buffer, in
one pass.

Expected values in every case come from tests/unreach_ref.py: the status bytes are the oracle's verify, the
REFUSED and address rules and the head bytes its own restatement of the header text, every reply checksum the
oracle's emit on the error frame.  All comparisons are exact: status, entries, the WHOLE arena (filled with the
sentinel 0xA5, so a stray store anywhere fails), and the batch buffer and the port map unchanged.  Each test
asserts that the classes it means to exercise occur in its batch."""
import numpy as np
import pytest

import oracle
from tests import cut_ref as C
from tests import pktgen as P
from tests import unreach_ref as R
from tests.test_echo_rule_cpu import BCAST
from tests.test_unreach_rule_cpu import outcome, sweep

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from smoltcp_amd import engine as E  # noqa: E402

NOCAPS = (0, 0, 0, 0, 0)
V4A, V4B = bytes([10, 1, 2, 3]), bytes([10, 4, 5, 6])
V6A, V6B = bytes(range(0x20, 0x30)), bytes(range(0x40, 0x50))
MCAST4, MCAST6 = bytes([224, 0, 0, 1]), bytes.fromhex("ff02") + bytes(13) + b"\x01"
# the launch shapes of the kernel's shape set, by the number set_shape takes: (G, U)
SHAPES = {0: (8, 6), 7: (8, 7), 1: (16, 3), 8: (16, 4), 4: (32, 4), 6: (64, 4)}
CLOSED, OPEN = 4000, 53           # a closed and an open port of PORTS
PORTS = E.make_port_map([OPEN, 67, 68, 5353])
UNKNOWN4, UNKNOWN6 = (47, 132, 89, 255, 0, 58), (47, 132, 89, 255, 59, 1)  # protocols / next headers nobody handles
FULL = R.REFUSED | R.ANSWERED | R.WRITTEN | R.SEND
PFULL = FULL | R.PORT


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    e = E.ChecksumEngine(0)
    yield e
    e.close()


# ---- packets ---------------------------------------------------------------------------------------

def ip4(rng, proto: int, payload: bytes, src=V4A, dst=V4B, ihl: int = 5, plain: bool = False) -> bytes:
    """An IPv4 packet; unless plain, with what the quoted header must not carry: random DSCP / ECN and ident,
    DF clear, a random TTL, NOP options."""
    if plain:
        return P.ipv4(src, dst, proto, payload)
    r = bytearray(P.ipv4(src, dst, proto, payload, ihl=ihl, options=bytes([1]) * (ihl * 4 - 20), flags_frag=0,
                         ident=int(rng.integers(0, 65536)), ttl=int(rng.integers(1, 256))))
    r[1] = int(rng.integers(0, 256))
    return bytes(r)


def ip6(rng, nh: int, payload: bytes, src=V6A, dst=V6B, plain: bool = False) -> bytes:
    """An IPv6 packet; unless plain, with a random traffic class, flow label and hop limit."""
    if plain:
        return P.ipv6(src, dst, nh, payload)
    r = bytearray(P.ipv6(src, dst, nh, payload, hop=int(rng.integers(1, 256))))
    r[0] = 0x60 | int(rng.integers(0, 16))
    r[1:4] = P.rand_bytes(rng, 3)
    return bytes(r)


def eth(r: bytes, mac_dst=None, mac_src=None) -> bytes:
    f = P.eth(r, 0x0800 if r[0] >> 4 == 4 else 0x86DD)
    return (mac_dst or f[0:6]) + (mac_src or f[6:12]) + f[12:]


def refused(rng, ver: int, kind: int, plen: int, port: bool, dport: int = CLOSED, trail: int = 0, **kw) -> bytes:
    """A record with an IP payload of plen bytes: a UDP datagram to dport (its last `trail` bytes behind the UDP
    length), or a payload of a protocol / next header nobody handles."""
    if port:
        pay = P.udp(int(rng.integers(1, 65536)), dport, P.rand_bytes(rng, plen - 8 - trail)) + P.rand_bytes(rng, trail)
        proto = 17
    else:
        pay = P.rand_bytes(rng, plen)
        proto = (UNKNOWN4 if ver == 4 else UNKNOWN6)[int(rng.integers(0, 6))]
    r = ip4(rng, proto, pay, **kw) if ver == 4 else ip6(rng, proto, pay, **kw)
    return eth(r) if kind == E.KIND_ETH else r


# ---- one call, compared exactly ----------------------------------------------------------------------

def _prepare(recs, kinds, rflags=0, caps=NOCAPS, cfg=None, ports=PORTS, fixed=None, offs=None, flips=(), patches=(),
             cap_adj=0, cap_abs=None, dst_mod=None, seed=0):
    """The batch buffer (every checksum filled by the oracle's emit, then `patches` = (record, byte, bytes)
    overwrite and `flips` = (record, byte, bit) corrupt single bits), slots back to back (dst_mod[i]: the slot's
    start at that residue mod 16, the gap showing the sentinel) with cap = the frame's length + cap_adj (cap_abs:
    that cap for all), and the reference's results."""
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
    for i, o, b in patches:
        buf[int(offs[i]) + o:int(offs[i]) + o + len(b)] = np.frombuffer(b, np.uint8)
    for i, o, bit in flips:
        buf[int(offs[i]) + o] ^= 1 << bit
    placed = [bytes(buf[int(o):int(o) + int(ln)]) for o, ln in zip(offs, lens)]
    need = R.frame_lens(placed, kinds_a, flags_a, ports, cfg)
    cap = np.maximum(need + cap_adj, 0) if cap_abs is None else np.full(n, cap_abs, np.int64)
    d_offs, pos = np.zeros(n, np.uint64), 3
    for i in range(n):
        if dst_mod is not None:
            pos += (int(dst_mod[i]) - pos) % 16
        d_offs[i] = pos
        pos += int(cap[i])
    slots = E.make_slots(d_offs, cap)
    st, ent, arena = R.expected(placed, kinds_a, flags_a, caps, cfg, ports, slots, pos + 21)
    return dict(buf=buf, offs=offs, lens=lens, kinds=kinds_a, flags=flags_a, fixed=fixed, caps=caps, cfg=cfg, ports=ports,
                slots=slots, status=st, entries=ent, arena=arena, fl=ent["flags"].astype(np.int64))


def _call(eng, b, shape=-1, blocks=0, stream=None):
    """The call on a prepared batch; every assertion of a case.  Returns the device arena."""
    eng.set_shape(shape)
    eng.set_max_blocks(blocks)
    try:
        batch, d, dv, dst, sd = C.upload(E, b["buf"], b["offs"], b["lens"], b["kinds"], b["flags"], b["fixed"], b["slots"],
                                         b["arena"].size)
        pm = torch.from_numpy(b["ports"].copy()).cuda() if b["ports"] is not None else None
        kw = dict(udp_open=pm, caps=b["caps"], cfg=b["cfg"])
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                st, ent = eng.verify_unreach_reply(dv, batch, dst, sd, stream=stream, **kw)
            stream.synchronize()
        else:
            st, ent = eng.verify_unreach_reply(dv, batch, dst, sd, **kw)
        launched = eng.last_launch()
        got_st, got_dst = st.cpu().numpy(), dst.cpu().numpy()
        got_ent = ent.cpu().numpy().reshape(-1).view(E.UNR_DTYPE)
        assert np.array_equal(d.cpu().numpy(), b["buf"]), "the batch buffer is only read"
        assert pm is None or np.array_equal(pm.cpu().numpy(), b["ports"]), "the port map is only read"
    finally:
        eng.set_shape(-1)
        eng.set_max_blocks(0)
    assert launched["kernel"] == "unreach" and launched["variant"] == 0, launched
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


def _frame(b, i: int) -> bytes:
    o = int(b["slots"][i]["dst_offset"])
    return bytes(b["arena"][o:o + int(b["entries"][i]["frame_len"])])


# ---- payload lengths around both cuts and the 16-byte grid ------------------------------------------------

PLENS = (0, 1, 7, 8, 9, 15, 16, 17, 31, 33, 527, 528, 529, 543, 1191, 1192, 1193, 1472)


@pytest.mark.parametrize("ver", [4, 6])
@pytest.mark.parametrize("kind", [E.KIND_IP, E.KIND_ETH])
def test_payload_lengths_around_both_cuts(eng, ver, kind):
    """Every P in the protocol / next-header form and, from 8 up, the port form, each at every record start mod
    16, the slots back to back at changing residues.  Every other UDP datagram longer than the cut carries a
    flipped bit in its last byte: the frame stops at the cut while the status reflects the bytes behind it."""
    rng = np.random.default_rng(10 * ver + kind)
    recs, offs, dmod, flips, pos = [], [], [], [], 0
    cut = R.DATA_V4 if ver == 4 else R.DATA_V6
    for plen in PLENS:
        for port in (False, True):
            if port and plen < 8:
                continue
            for sa in range(16):
                r = refused(rng, ver, kind, plen, port)
                pos += (sa - pos) % 16  # the device buffers are 16-byte aligned
                offs.append(pos)
                if port and plen > cut and sa % 2:
                    flips.append((len(recs), len(r) - 1, sa % 8))
                recs.append(r)
                dmod.append((5 * sa + len(recs) // 16) % 16)
                pos += len(r)
    b = _run(eng, recs, kind, offs=np.array(offs, np.uint64), dst_mod=dmod, flips=flips, seed=ver)
    hl = (14 if kind == E.KIND_ETH else 0) + (48 if ver == 4 else 88)
    assert (b["entries"]["head_len"] == hl).all() and len(set(dmod)) == 16
    assert sorted(set((b["entries"]["frame_len"] - hl).tolist())) == sorted({min(p, cut) for p in PLENS})
    assert int(b["entries"]["frame_len"].max()) == hl + cut
    flipped = np.zeros(len(recs), bool)
    flipped[[f[0] for f in flips]] = True
    assert len(flips) >= 8 and (b["fl"][flipped] == PFULL & ~R.SEND).all()
    assert set(b["fl"][~flipped].tolist()) == {FULL, PFULL}


# ---- a UDP length shorter than P ---------------------------------------------------------------------------

def _short_udp(ver, kind):
    """(records, the UDP length per record, the trailing length per record): UDP lengths odd and even, the
    trailing bytes below the cut, above it and across it."""
    rng = np.random.default_rng(20 + ver + kind)
    cut = R.DATA_V4 if ver == 4 else R.DATA_V6
    recs, uls, trails = [], [], []
    for ul in (8, 9, 21, 28, cut - 100, cut - 99, cut - 1, cut, cut + 1, cut + 172, cut + 173):
        for trail in (1, 2, 17, 600):
            for _ in range(2):
                recs.append(refused(rng, ver, kind, ul + trail, True, trail=trail))
                uls.append(ul)
                trails.append(trail)
    return recs, np.array(uls), np.array(trails), cut


@pytest.mark.parametrize("ver", [4, 6])
@pytest.mark.parametrize("kind", [E.KIND_IP, E.KIND_ETH])
def test_udp_length_shorter_than_the_ip_payload(eng, ver, kind):
    """The bytes behind the UDP length are quoted and summed into the reply, and are no part of the verdict."""
    recs, uls, trails, cut = _short_udp(ver, kind)
    n = len(recs)
    off = len(recs[0]) - int(uls[0] + trails[0])  # the IP payload's offset: the same in every record
    base = _run(eng, recs, kind, seed=21)
    assert (base["fl"] == PFULL).all()
    assert ((uls + trails <= cut).any() and (uls >= cut).any() and ((uls < cut) & (uls + trails > cut)).any())
    hl = int(base["entries"]["head_len"][0])
    l4ck = hl - (26 if ver == 4 else 46)  # the ICMP checksum's place in the frame

    # a bit flipped in the trailing bytes below the cut: the reply and its checksum change, ACCEPT and SEND stay
    who = [i for i in range(n) if uls[i] < cut]
    b = _run(eng, recs, kind, flips=[(i, off + int(uls[i]), 3) for i in who], seed=21)
    assert len(who) >= 20 and (b["fl"] == PFULL).all() and np.array_equal(b["status"], base["status"])
    for i in who:
        f0, f1 = _frame(base, i), _frame(b, i)
        assert f0[hl + int(uls[i])] ^ f1[hl + int(uls[i])] == 8 and f0[l4ck:l4ck + 2] != f1[l4ck:l4ck + 2]

    # a bit flipped in the UDP span past the cut: SEND goes, the frame's bytes stay
    who = [i for i in range(n) if uls[i] > cut]
    b = _run(eng, recs, kind, flips=[(i, off + int(uls[i]) - 1, 5) for i in who], seed=21)
    assert len(who) >= 16
    for i in range(n):
        assert int(b["fl"][i]) == (PFULL & ~R.SEND if i in who else PFULL) and _frame(b, i) == _frame(base, i)

    # a bit flipped in the UDP span below the cut: the frame's data and ICMP checksum change, SEND goes
    who = [i for i in range(n) if uls[i] > 8]
    at = [min(int(uls[i]), cut) - 1 for i in range(n)]
    b = _run(eng, recs, kind, flips=[(i, off + at[i], 0) for i in who], seed=21)
    for i in who:
        f0, f1 = _frame(base, i), _frame(b, i)
        assert int(b["fl"][i]) == PFULL & ~R.SEND and f0[hl + at[i]] ^ f1[hl + at[i]] == 1 and f0[l4ck:l4ck + 2] != f1[l4ck:l4ck + 2]


# ---- headers are rebuilt, not copied ------------------------------------------------------------------------

def test_headers_are_rebuilt_not_copied(eng):
    """IPv4 requests with IHL 6 and 15, random DSCP / ECN, ident, DF clear and random TTL; IPv6 with a traffic
    class, a flow label and a random hop limit: the quoted header carries the TTL / hop limit and the protocol
    only, and its length field is the full P also when the data is cut."""
    rng = np.random.default_rng(31)
    recs, kinds, plens = [], [], []
    for i in range(192):
        plen = (8, 40, 528, 529, 1192, 1193, 1400, 77)[i % 8]
        kind = E.KIND_ETH if (i // 8) % 2 else E.KIND_IP
        ver = 4 if (i // 16) % 2 else 6
        kw = {"ihl": (6, 15, 5)[(i // 32) % 3]} if ver == 4 else {}
        recs.append(refused(rng, ver, kind, plen, bool(i % 3), **kw))
        kinds.append(kind)
        plens.append(plen)
    b = _run(eng, recs, kinds, seed=32)
    assert set(b["fl"].tolist()) == {FULL, PFULL}
    cutseen = 0
    for i, r in enumerate(recs):
        e = 14 if kinds[i] == E.KIND_ETH else 0
        f = _frame(b, i)
        if r[e] >> 4 == 4:
            q = f[e + 28:e + 48]
            assert q[:2] == b"\x45\x00" and q[2:4] == P.be16(20 + plens[i]) and q[4:8] == b"\x00\x00\x40\x00"
            assert q[8:10] == r[e + 8:e + 10] and q[12:20] == r[e + 12:e + 20] and r[e + 6] & 0x40 == 0
            cutseen += plens[i] > R.DATA_V4 and len(f) == e + 48 + R.DATA_V4
        else:
            q = f[e + 48:e + 88]
            assert q[:4] == b"\x60\x00\x00\x00" and q[4:6] == P.be16(plens[i]) and q[6] == r[e + 6] and q[7] == r[e + 7]
            assert q[8:40] == r[e + 8:e + 40]
            cutseen += plens[i] > R.DATA_V6 and len(f) == e + 88 + R.DATA_V6
    assert cutseen >= 30
    assert {int(r[14 if k == E.KIND_ETH else 0]) & 15 for r, k in zip(recs, kinds) if r[14 if k == E.KIND_ETH else 0] >> 4 == 4} == {5, 6, 15}


# ---- the port map ---------------------------------------------------------------------------------------

PROBE_PORTS = (0, 1, 7, 8, 31, 32, 255, 256, 32767, 32768, 65535)


def _alternating(complement: bool) -> np.ndarray:
    """Bits that alternate from port to port, from byte to byte and from 2 KiB to 2 KiB of the map."""
    p = np.arange(65536)
    bit = ((p ^ (p >> 3) ^ (p >> 14)) & 1) ^ int(complement)
    return np.packbits(bit.astype(np.uint8), bitorder="little")


@pytest.mark.parametrize("which", ["null", "alternating", "complement"])
def test_port_map(eng, which):
    rng = np.random.default_rng(41)
    ports = None if which == "null" else _alternating(which == "complement")
    recs, kinds, dports = [], [], []
    for i in range(len(PROBE_PORTS) * 8):
        dp = PROBE_PORTS[i % len(PROBE_PORTS)]
        kinds.append(E.KIND_ETH if i % 2 else E.KIND_IP)
        recs.append(refused(rng, 4 if (i // 2) % 2 else 6, kinds[-1], 30, True, dport=dp))
        dports.append(dp)
    recs.append(refused(rng, 4, E.KIND_IP, 30, False))  # the protocol form needs no map
    kinds.append(E.KIND_IP)
    b = _run(eng, recs, kinds, ports=ports, seed=42)
    assert b["fl"][-1] == FULL
    for i, dp in enumerate(dports):
        want = 0 if ports is None or dp == 0 or R.port_open(ports, dp) else PFULL
        assert int(b["fl"][i]) == want, (dp, which)
        assert bool(b["status"][i] & E.ST_MALFORMED) == (dp == 0)
    if ports is not None:
        closed = [dp for dp in PROBE_PORTS[1:] if not R.port_open(ports, dp)]
        assert 3 <= len(closed) <= 7, closed  # both outcomes among the probes, and they swap under the complement
        assert E.make_port_map([p for p in range(65536) if R.port_open(ports, p)]).tobytes() == ports.tobytes()


# ---- checksums and caps -----------------------------------------------------------------------------------

def _caps_batch(ver):
    """40 records: both forms and kinds; every fourth with a flipped payload bit, every fifth IPv4 one with a
    flipped header-checksum bit.  Records 0 and 1 (IP, Ethernet) are left whole."""
    rng = np.random.default_rng(50 + ver)
    recs, kinds, flips = [], [], []
    for i in range(40):
        kinds.append(E.KIND_ETH if i % 2 else E.KIND_IP)
        plen = int(rng.integers(9, 700))
        r = refused(rng, ver, kinds[-1], plen, i % 4 != 2, plain=True)
        recs.append(r)
        e = 14 if i % 2 else 0
        if i % 4 == 3:
            flips.append((i, len(r) - 1 - int(rng.integers(0, plen - 8)), i % 8))
        elif i % 5 == 4 and ver == 4:
            flips.append((i, e + 10 + i % 2, i % 8))
    return recs, kinds, flips


@pytest.mark.parametrize("ipv4", [0, 1, 2, 3])
@pytest.mark.parametrize("icmpv4", [0, 1, 2, 3])
@pytest.mark.parametrize("udp", [0, 1, 2, 3])
def test_caps_ipv4(eng, ipv4, icmpv4, udp):
    recs, kinds, flips = _caps_batch(4)
    b = _run(eng, recs, kinds, caps=(ipv4, udp, 3, icmpv4, 3), flips=flips, seed=51)
    assert (b["fl"] & R.WRITTEN).all()
    rx_any = ipv4 in (0, 1) or udp in (0, 1)
    assert ((b["fl"] & R.SEND) == 0).any() == rx_any  # written, not to be sent: a gate that is on caught the record
    # the frame's fields are zero exactly when tx is off
    for i in (0, 1):
        f, e = _frame(b, i), 14 * i
        assert any(f[e + 10:e + 12]) == (ipv4 in (0, 2)) == any(f[e + 38:e + 40])
        assert any(f[e + 22:e + 24]) == (icmpv4 in (0, 2))


@pytest.mark.parametrize("icmpv6", [0, 1, 2, 3])
@pytest.mark.parametrize("udp", [0, 1, 2, 3])
def test_caps_ipv6(eng, icmpv6, udp):
    recs, kinds, flips = _caps_batch(6)
    b = _run(eng, recs, kinds, caps=(3, udp, 3, 3, icmpv6), flips=flips, seed=52)
    assert (b["fl"] & R.WRITTEN).all()
    assert ((b["fl"] & R.SEND) == 0).any() == (udp in (0, 1))
    for i in (0, 1):
        f, e = _frame(b, i), 14 * i
        assert any(f[e + 42:e + 44]) == (icmpv6 in (0, 2))


def test_zero_checksum_fields_and_extreme_data(eng):
    """A UDP / IPv4 request with a zero checksum field is accepted and answered to be sent; a UDP / IPv6 one is
    refused and written, and sent exactly when verify accepts it; a bad IPv4 header checksum under rx: no SEND;
    data of all zero bytes and of all 0xff bytes."""
    rng = np.random.default_rng(55)
    recs, kinds, patches, flips, want = [], [], [], [], []
    for i in range(48):
        kind = E.KIND_ETH if i % 2 else E.KIND_IP
        e = 14 if i % 2 else 0
        m = (i // 2) % 6
        body = (bytes(200), b"\xff" * 200, P.rand_bytes(rng, 200))[i % 3]
        if m == 0:    # UDP / IPv4, checksum field zero
            r = P.ipv4(V4A, V4B, 17, P.udp(9, CLOSED, body))
            patches.append((i, e + 26, b"\0\0"))
            want.append(PFULL)
        elif m == 1:  # UDP / IPv6, checksum field zero: refused and written; the status is verify's, and the
            # reference accepts a zero field over IPv6 as well (UdpPacket::verify_checksum, udp.rs:138-140, comes
            # before the IPv4-only arm of UdpRepr::parse, udp.rs:250-256), so SEND follows ACCEPT here too
            r = P.ipv6(V6A, V6B, 17, P.udp(9, CLOSED, body))
            patches.append((i, e + 46, b"\0\0"))
            want.append(PFULL)
        elif m == 2:  # a bad IPv4 header checksum
            r = P.ipv4(V4A, V4B, 17 if i % 4 < 2 else 47, P.udp(9, CLOSED, body))
            flips.append((i, e + 10, 2))
            want.append((PFULL if i % 4 < 2 else FULL) & ~R.SEND)
        elif m == 3:  # all-zero / all-0xff data in the protocol form: the whole payload
            r = P.ipv4(V4A, V4B, 47, body)
            want.append(FULL)
        elif m == 4:
            r = P.ipv6(V6A, V6B, 47, body + body[:1])
            want.append(FULL)
        else:         # a UDP datagram that is all 0xff behind the IPv4 header
            r = P.ipv4(V4A, V4B, 17, b"\xff" * 8 + body)
            patches.append((i, e + 20, b"\xff" * 4 + P.be16(208)))
            want.append(None)
        recs.append(eth(r) if i % 2 else r)
        kinds.append(kind)
    ports = _alternating(False) & 0  # every port closed
    b = _run(eng, recs, kinds, ports=ports, patches=patches, flips=flips, seed=56)
    for i, w in enumerate(want):
        if w is not None:
            assert int(b["fl"][i]) == w, (i, hex(int(b["fl"][i])), hex(w))
        else:
            assert b["fl"][i] & R.WRITTEN and b["fl"][i] & R.PORT


# ---- the address rule -------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_cfg", [False, True])
def test_address_rule_table(eng, with_cfg):
    """One record per row of the rule's table (tests/test_unreach_rule_cpu.py's sweep at one P, both forms, no
    Hop-by-Hop header), with cfg NULL and with bcast_v4 set.  It includes the IPv4 broadcast destination that the
    echo call marks HOST and this call leaves unanswered."""
    recs, kinds, want = [], [], []
    for case in sweep():
        kind, ver, md, ms, et, s, d, bc, proto, hbh, closed, plen, hop = case
        if plen != 528 or (bc is not None) != with_cfg or hbh or proto not in (17, 47) or not closed:
            continue
        pay = P.udp(9, CLOSED, bytes(range(256)) * 2 + bytes(8)) if proto == 17 else bytes(range(256)) * 2 + bytes(16)
        r = P.ipv4(s, d, proto, pay, ttl=hop or 1) if ver == 4 else P.ipv6(s, d, proto, pay, hop=hop)
        recs.append(md + ms + et + r if kind == E.KIND_ETH else r)
        kinds.append(kind)
        want.append(outcome(*case)[0])
    b = _run(eng, recs, kinds, cfg=BCAST if with_cfg else None, seed=61)
    assert ((b["fl"] & ~(R.WRITTEN | R.SEND)) == np.array(want)).all()
    assert len(recs) == 2 * (7 * 7 + 5 * 5) * 4 * 2
    for fl in (FULL, PFULL, R.REFUSED, R.REFUSED | R.PORT, R.REFUSED | R.HOST, R.REFUSED | R.PORT | R.HOST):
        assert _has(b, fl, 20), hex(fl)
    i = next(i for i, r in enumerate(recs) if kinds[i] == E.KIND_IP and r[0] >> 4 == 4 and r[12:16] == V4A and r[16:20] == b"\xff" * 4)
    assert b["fl"][i] & ~R.PORT == R.REFUSED and not b["entries"][i]["frame_len"]


# ---- records that are not refused ---------------------------------------------------------------------------

def _not_refused(rng):
    """(record, kind, record flags) of everything that must leave an all-zero entry and an untouched slot."""
    pay = P.rand_bytes(rng, int(rng.integers(8, 200)))
    inner = P.ipv4(V4B, V4A, 17, P.udp(7, 9, pay[:8]))
    u4, u6 = P.ipv4(V4A, V4B, 17, P.udp(7, CLOSED, pay)), P.ipv6(V6A, V6B, 17, P.udp(7, CLOSED, pay))
    x4 = P.ipv4(V4A, V4B, 47, pay)
    out = [
        (P.ipv4(V4A, V4B, 6, P.tcp(7, 9, pay)), E.KIND_IP, 0),                     # TCP
        (P.ipv6(V6A, V6B, 6, P.tcp(7, 9, pay)), E.KIND_IP, 0),
        (P.ipv4(V4A, V4B, 1, P.icmp_echo(8, pay)), E.KIND_IP, 0),                  # echo requests
        (P.ipv6(V6A, V6B, 58, P.icmp_echo(128, pay)), E.KIND_IP, 0),
        (P.ipv4(V4A, V4B, 1, P.icmp4_error(3, 3, inner)), E.KIND_IP, 0),           # ICMP errors
        (P.ipv6(V6A, V6B, 58, bytes([1, 4, 0, 0, 0, 0, 0, 0]) + u6[:48]), E.KIND_IP, 0),
        (P.ipv4(V4A, V4B, 2, bytes([0x11, 0, 0, 0, 224, 0, 0, 1])), E.KIND_IP, 0),  # IGMP
        (P.ipv4(V4A, V4B, 17, u4[20:], flags_frag=0x2000), E.KIND_IP, 0),          # fragments: MF; an offset
        (P.ipv4(V4A, V4B, 47, pay, flags_frag=0x0003), E.KIND_IP, 0),
        (u4, E.KIND_IP, E.REC_IPHDR_ONLY),
        (x4, E.KIND_IP, E.REC_IPHDR_ONLY),
        (P.ipv6(V6A, V6B, 47, pay), E.KIND_IP, E.REC_IPHDR_ONLY),
        (x4, E.KIND_RAW, 0),
        (P.eth(x4, 0x0806), E.KIND_ETH, 0),                                        # a non-IP ethertype
        (P.eth(u4, 0x86DD), E.KIND_ETH, 0),                                        # ethertype / version mismatch
        (x4[:19], E.KIND_IP, 0),                                                   # truncated IP headers
        (P.ipv4(V4A, V4B, 47, pay, total_len=20 + len(pay) + 1), E.KIND_IP, 0),
        (eth(P.ipv6(V6A, V6B, 47, pay)[:39]), E.KIND_ETH, 0),
        (P.ipv6(V6A, V6B, 47, pay, payload_len=len(pay) + 1), E.KIND_IP, 0),
        (P.ipv4(V4A, V4B, 17, u4[20:27]), E.KIND_IP, 0),                           # truncated UDP headers
        (P.ipv6(V6A, V6B, 17, P.udp(7, CLOSED, pay, length=7)), E.KIND_IP, 0),
        (P.ipv4(V4A, V4B, 17, P.udp(7, CLOSED, pay, length=9 + len(pay))), E.KIND_IP, 0),
        (P.ipv4(V4A, V4B, 17, P.udp(7, 0, pay)), E.KIND_IP, 0),                    # destination port 0
        (P.ipv4(V4A, V4B, 17, P.udp(7, OPEN, pay)), E.KIND_IP, 0),                 # UDP to an open port
        (eth(P.ipv6(V6A, V6B, 17, P.udp(7, 5353, pay))), E.KIND_ETH, 0),
        (P.ipv6(V6A, V6B, 0, P.hbh_opts(17, bytes([0xC2, 0])) + u6[40:]), E.KIND_IP, 0),  # a Hop-by-Hop drop
        (P.ipv6(V6A, V6B, 0, P.hbh(17, 0, rng) + P.udp(7, OPEN, pay)), E.KIND_IP, 0),     # open behind Hop-by-Hop
    ]
    return out


def _hbh_refused(rng, kind):
    """Hop-by-Hop-led records the host answers: UDP to a closed port, an unknown next header, a second
    Hop-by-Hop header; one of them behind a header longer than the kernel's window."""
    pay = P.rand_bytes(rng, int(rng.integers(8, 100)))
    out = [P.ipv6(V6A, V6B, 0, P.hbh(17, 0, rng) + P.udp(7, CLOSED, pay)),
           P.ipv6(V6A, V6B, 0, P.hbh(17, 20, rng) + P.udp(7, CLOSED, pay)),
           P.ipv6(V6A, V6B, 0, P.hbh(47, 1, rng) + pay),
           P.ipv6(V6A, V6B, 0, P.hbh(0, 0, rng) + P.hbh(17, 0, rng) + pay)]
    return [eth(r) if kind == E.KIND_ETH else r for r in out]


def test_records_that_are_not_refused_between_refused_ones(eng):
    rng = np.random.default_rng(71)
    recs, kinds, rflags, cls = [], [], [], []
    for rep in range(6):
        for r, k, f in _not_refused(rng):
            recs.append(r), kinds.append(k), rflags.append(f), cls.append(0)
            kind = E.KIND_ETH if len(recs) % 4 < 2 else E.KIND_IP
            recs.append(refused(rng, 4 if len(recs) % 8 < 4 else 6, kind, int(rng.integers(8, 90)), bool(len(recs) % 3)))
            kinds.append(kind), rflags.append(0), cls.append(1)
        for r in _hbh_refused(rng, E.KIND_ETH if rep % 2 else E.KIND_IP):
            recs.append(r), kinds.append(E.KIND_ETH if rep % 2 else E.KIND_IP), rflags.append(0), cls.append(2)
    b = _run(eng, recs, kinds, rflags=rflags, seed=72)
    cls = np.array(cls)
    assert set(b["fl"][cls == 1].tolist()) == {FULL, PFULL}
    assert not b["entries"][cls == 0].view(np.uint8).any(), "a record that is not refused has an entry"
    assert set(b["fl"][cls == 2].tolist()) == {R.REFUSED | R.HOST, R.REFUSED | R.HOST | R.PORT}
    h = b["entries"][cls == 2]
    assert not h["frame_len"].any() and not h["head_len"].any() and set(h["data_off"].tolist()) == {40, 54}
    other = b["status"][cls == 0]  # accepted with every gate passed, unsupported, malformed
    assert (other & (E.ST_MALFORMED | E.ST_UNSUPPORTED) == 0).any()
    assert (other & E.ST_MALFORMED).any() and (other & E.ST_UNSUPPORTED).any()


# ---- the cap ------------------------------------------------------------------------------------------------

def _mixed_refused(rng, n, kind, maxlen):
    return [refused(rng, 4 if i % 2 else 6, kind, int(rng.integers(8, maxlen)) if i % 3 else int(rng.integers(8, 60)),
                    bool(i % 4)) for i in range(n)]


@pytest.mark.parametrize("mode", ["fit", "one_short", "zero"])
def test_cap(eng, mode):
    rng = np.random.default_rng(81)
    recs = _mixed_refused(rng, 160, E.KIND_ETH, 1473)
    dmod = [(7 * i) % 16 for i in range(160)]
    b = _run(eng, recs, E.KIND_ETH, seed=82, dst_mod=dmod, **({"cap_adj": 0} if mode == "fit" else {"cap_adj": -1}
                                                           if mode == "one_short" else {"cap_abs": 0}))
    if mode == "fit":
        assert set(b["fl"].tolist()) == {FULL, PFULL}
    else:  # answered, not written: the lengths reported, the arena untouched
        assert set(b["fl"].tolist()) == {R.REFUSED | R.ANSWERED, R.REFUSED | R.ANSWERED | R.PORT}
        assert (b["arena"] == C.SENTINEL).all()
        assert (b["entries"]["frame_len"] >= 62 + 8).all() and (b["entries"]["head_len"] >= 62).all()


# ---- every launch shape -------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("fixed", [False, True])
def test_every_shape(eng, shape, fixed):
    """Each shape of the shape set forced through set_shape.  The fixed-stride batch's stride exceeds every
    datagram: the random bytes behind a datagram are neither summed nor quoted."""
    rng = np.random.default_rng(100 + shape)
    kind = E.KIND_ETH if shape % 2 else E.KIND_IP
    recs = _mixed_refused(rng, 200, kind, 1400 if fixed else 3000)
    flips = [(i, len(recs[i]) - 1 - int(rng.integers(0, 8)), int(rng.integers(0, 8))) for i in range(5, 200, 13) if i % 4]
    b = _run(eng, recs, kind, shape=shape, fixed=(1531, 7) if fixed else None, flips=flips, seed=shape)
    assert _has(b, FULL, 40) and _has(b, PFULL, 100) and _has(b, PFULL & ~R.SEND, 8)


def test_ethernet_padding_is_not_quoted(eng):
    """60-byte Ethernet frames at a fixed stride: one half carry an 18-byte UDP datagram (the frame exactly), the
    other half a 10-byte one and 8 bytes of padding, which the frame must not carry."""
    rng = np.random.default_rng(91)
    recs = []
    for i in range(120):
        r = eth(P.ipv4(V4A, V4B, 17, P.udp(9, CLOSED, P.rand_bytes(rng, 10 if i % 2 else 2))))
        recs.append(r + P.rand_bytes(rng, 60 - len(r)))
    b = _run(eng, recs, E.KIND_ETH, fixed=(60, 4), seed=92)
    assert (b["fl"] == PFULL).all()
    assert sorted(set(b["entries"]["frame_len"].tolist())) == [62 + 10, 62 + 18]


# ---- the grid stride, a side stream, the empty batch, a long fixed-stride batch ------------------------------

def _mix(rng, n):
    """Mixed records of a descriptor batch: (records, kinds, record flags, flips, cap adjustment per record)."""
    recs, kinds, rflags, flips, adj = [], [], [], [], np.zeros(n, np.int64)
    others, hbhs = [], []
    for i in range(n):
        c = int(rng.integers(0, 100))
        kind = E.KIND_ETH if rng.integers(0, 2) else E.KIND_IP
        ver = 4 if rng.integers(0, 2) else 6
        port = bool(rng.integers(0, 3))
        plen = int(rng.integers(8, 1473)) if rng.integers(0, 4) else int(rng.integers(8, 100))
        trail = int(rng.integers(0, min(plen - 8, 40) + 1)) if port and rng.integers(0, 4) == 0 else 0
        f = 0
        if c < 45:  # answered and sent
            r = refused(rng, ver, kind, plen, port, trail=trail)
        elif c < 53:  # a corrupted request: written, not sent
            r = refused(rng, ver, kind, plen, True)
            flips.append((i, len(r) - 1 - int(rng.integers(0, plen - 8 + 1)), int(rng.integers(0, 8))))
        elif c < 59:  # a slot too short
            r = refused(rng, ver, kind, plen, port)
            adj[i] = -1 - int(rng.integers(0, 40))
        elif c < 66:  # the host's: a multicast IPv6 destination, a group MAC, a Hop-by-Hop header
            m = int(rng.integers(0, 3))
            if m == 0:
                r = refused(rng, 6, kind, plen, port, dst=MCAST6)
            elif m == 1:
                r = refused(rng, ver, E.KIND_IP, plen, port)
                kind = E.KIND_ETH
                r = eth(r, mac_dst=bytes([0xFF] * 6)) if rng.integers(0, 2) else eth(r, mac_src=bytes([0x03, 0, 0, 0, 0, 9]))
            else:
                if not hbhs:
                    hbhs = _hbh_refused(rng, E.KIND_IP)
                r, kind = hbhs.pop(), E.KIND_IP
        elif c < 73:  # nobody answers: a broadcast / multicast IPv4 destination, a non-unicast source
            m = int(rng.integers(0, 3))
            kw = {"dst": (MCAST4, b"\xff" * 4)[m % 2]} if m < 2 and ver == 4 else {"src": bytes(4) if ver == 4 else MCAST6}
            r = refused(rng, ver, kind, plen, port, **kw)
        else:  # not refused
            if not others:
                others = _not_refused(rng)
                rng.shuffle(others)
            r, kind, f = others.pop()
        recs.append(r), kinds.append(kind), rflags.append(f)
    return recs, kinds, rflags, flips, adj


def test_grid_stride_over_one_workgroup(eng):
    rng = np.random.default_rng(101)
    recs, kinds, rflags, flips, adj = _mix(rng, 600)
    b = _run(eng, recs, kinds, rflags=rflags, flips=flips, cap_adj=adj, blocks=1, seed=102)
    assert _has(b, PFULL, 100) and _has(b, FULL, 50) and _has(b, 0, 60)


def test_side_stream_and_empty_batch(eng):
    rng = np.random.default_rng(111)
    recs, kinds, rflags, flips, adj = _mix(rng, 300)
    b = _run(eng, recs, kinds, rflags=rflags, flips=flips, cap_adj=adj, stream=torch.cuda.Stream(), seed=112)
    assert _has(b, PFULL, 50)
    e = torch.zeros(64, dtype=torch.uint8, device="cuda")
    st, ent = eng.verify_unreach_reply(e, E.Batch.fixed(0, 64, 64, E.KIND_IP), e, e)
    assert st.numel() == 0 and ent.numel() == 0


def test_4099_fixed_stride_probes(eng):
    """70-byte UDP probes over Ethernet at a fixed stride, nine in ten to closed ports, more records than one grid
    pass of small workgroups holds at the default shape."""
    rng = np.random.default_rng(121)
    recs = [eth(P.ipv4(V4A, V4B, 17, P.udp(40000 + i % 1000, OPEN if i % 10 == 9 else 1024 + i, P.rand_bytes(rng, 28)),
                       ttl=1 + i % 255)) for i in range(4099)]
    assert len(recs[0]) == 70
    flips = [(i, 69 - i % 20, i % 8) for i in range(3, 4099, 16)]
    b = _run(eng, recs, E.KIND_ETH, fixed=(70, 2), flips=flips, seed=122)
    assert _has(b, PFULL, 3300) and _has(b, PFULL & ~R.SEND, 200) and _has(b, 0, 400)
    assert set(b["entries"]["frame_len"].tolist()) == {0, 62 + 36}


# ---- round trip ---------------------------------------------------------------------------------------------

def test_written_frames_verify(eng):
    """The written frames of a batch fed back as a descriptor batch: every one passes verify with rx on, and
    none is refused in turn."""
    rng = np.random.default_rng(131)
    recs, kinds = [], []
    for i in range(300):
        kinds.append(E.KIND_ETH if i % 2 else E.KIND_IP)
        recs.append(refused(rng, 4 if i % 4 < 2 else 6, kinds[-1], int(rng.integers(8, 1473)) if i % 5 else 8 + i % 7, bool(i % 3)))
    b = _prepare(recs, kinds, seed=132)
    dst = _call(eng, b)
    w = (b["fl"] & R.WRITTEN) != 0
    assert w.all()
    back = E.Batch.from_records(b["slots"]["dst_offset"][w], b["entries"]["frame_len"][w], b["kinds"][w], "cuda:0")
    st = eng.verify(dst, back).cpu().numpy()
    assert (st & E.ST_ACCEPT).all() and (st & E.ST_IP_VALID).all() and (st & E.ST_L4_VALID).all()
    slots = torch.zeros(16 * int(w.sum()), dtype=torch.uint8, device="cuda")
    _, ent = eng.verify_unreach_reply(dst.clone(), back, dst, slots, udp_open=torch.zeros(8192, dtype=torch.uint8, device="cuda"))
    assert not ent.cpu().numpy().any()


# ---- randomized mix -----------------------------------------------------------------------------------------

MIX_SEED, MIX_N = 2025, 2048
# the least each class must hold: what the reference gives for MIX_SEED, rounded down to a round figure
MIX_FLOORS = {"sent": 800, "written, not sent": 100, "answered, not written": 60, "the host's": 60, "nobody answers": 60,
              "not refused": 300}


def mix_census(b):
    fl = b["fl"]
    return {"sent": int(((fl & R.SEND) != 0).sum()),
            "written, not sent": int((((fl & R.WRITTEN) != 0) & ((fl & R.SEND) == 0)).sum()),
            "answered, not written": int((((fl & R.ANSWERED) != 0) & ((fl & R.WRITTEN) == 0)).sum()),
            "the host's": int(((fl & R.HOST) != 0).sum()),
            "nobody answers": int(((fl & ~R.PORT) == R.REFUSED).sum()),
            "not refused": int((fl == 0).sum())}


def mix_batch():
    rng = np.random.default_rng(MIX_SEED)
    recs, kinds, rflags, flips, adj = _mix(rng, MIX_N)
    return _prepare(recs, kinds, rflags=rflags, flips=flips, cap_adj=adj, seed=MIX_SEED + 1)


def test_randomized_mix(eng):
    b = mix_batch()
    census = mix_census(b)
    for name, floor in MIX_FLOORS.items():
        assert census[name] >= floor, f"the mix holds {census[name]} records of class '{name}', fewer than {floor}"
    assert sum(census.values()) == MIX_N
    assert {fl & ~R.PORT for fl in b["fl"].tolist()} == {FULL, FULL & ~R.SEND, R.REFUSED | R.ANSWERED, R.REFUSED | R.HOST,
                                                        R.REFUSED, 0}
    _call(eng, b)
