"""GPU parity of verify_udp_enqueue (smol_csum_batch_verify_udp_enqueue): verify's status bytes, one
smol_csum_udprx_t per record, one smol_csum_udpsockout_t per group, the metadata entries, and every UDP
datagram's payload put where its socket's PacketBuffer::enqueue places it, in one pass.

Every case compares exactly:
  1. the status bytes with oracle.batch_verify, and with eng.verify on the same batch;
  2. the record and group entries with tests/udp_enqueue_ref.py;
  3. the WHOLE d_meta array, filled with 0x5A beforehand: the entries the accepted layout enqueues hold the
     model's bytes, every other entry keeps its fill;
  4. the WHOLE destination arena, filled with the sentinel 0xA5 beforehand: a byte of an ENQUEUED range holds
     its payload byte, a byte that lies in a speculative range and in no accepted one holds the sentinel or
     the speculative byte, every other byte holds the sentinel;
  5. the batch buffer: it is only read;
and asserts that the launch was udprx_kernel.  Status bytes and record entries of records the call must not
write keep their fill."""
import numpy as np
import pytest

import oracle
from tests import pktgen as P
from tests import udp_enqueue_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from smoltcp_amd import engine as E  # noqa: E402

NOCAPS = (0, 0, 0, 0, 0)
PRE = 0x5A  # the fill of the status, entry and metadata tensors: bytes the call must not write keep it
A4, B4 = bytes([10, 1, 2, 3]), bytes([10, 4, 5, 6])
A6, B6 = bytes(range(0x20, 0x30)), bytes(range(0x40, 0x50))
PORT = 5000
UDP, ENQ, FULL, PADDED, REST = E.URX_UDP, E.URX_ENQUEUED, E.URX_FULL, E.URX_PADDED, E.URX_RESTORED


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    e = E.ChecksumEngine(0)
    yield e
    e.close()


def dgram(payload, dport=PORT, sport=4321, v6=False, eth=True, pad=0, options=None, hbh=None, src=None, dst=None):
    """One UDP frame (checksums 0: the oracle's emit fills them); pad: Ethernet padding after the IP packet;
    options: IPv4 options (a multiple of 4 bytes); hbh: a Hop-by-Hop header in front of UDP."""
    u = P.udp(sport, dport, payload)
    if v6:
        ip = P.ipv6(src or A6, dst or B6, 0 if hbh is not None else 17, (hbh or b"") + u)
    else:
        ip = P.ipv4(src or A4, dst or B4, 17, u, ihl=5 + len(options or b"") // 4, options=options)
    return (P.eth(ip, 0x86DD if v6 else 0x0800) if eth else ip) + bytes(pad)


def rnd(seed, *sizes):
    rng = np.random.default_rng(seed)
    return [P.rand_bytes(rng, s) for s in sizes]


class Socks:
    """Sockets whose payload rings lie one after the other in the arena (gap bytes between them, 0: back to
    back) and whose metadata rings lie one after the other in d_meta, one unused entry between them."""

    def __init__(self, start=3, gap=0):
        self.pos, self.gap, self.mpos, self.rows = start, gap, 1, []

    def add(self, P_, M, pr=0, pl=0, mr=0, ml=0, port=PORT, reserved=(0, 0, 0), gap=None):
        self.pos += self.gap if gap is None else gap
        self.rows.append((self.pos, self.mpos, P_, pr, pl, M, mr, ml, port, reserved))
        self.pos += P_
        self.mpos += M + 1
        return len(self.rows) - 1

    def socks(self):
        s = E.make_udpsocks(*[[r[i] for r in self.rows] for i in range(9)])
        s["reserved"] = [r[9] for r in self.rows]
        return s, self.pos + 19, self.mpos + 1


def _model(recs, groups, socks, kinds=E.KIND_ETH, rflags=0, caps=NOCAPS, fixed=None, flips=(), zero=(), gap_seed=1):
    """The batch as the device gets it and what the model expects of the call: (buf, offs, lens, kinds, flags,
    groups, socks array, expected dict with "status")."""
    n = len(recs)
    groups = [tuple(g) + (0,) * (3 - len(g)) for g in groups]
    kinds_a = np.broadcast_to(np.asarray(kinds, np.uint8), (n,)).copy()
    flags_a = np.broadcast_to(np.asarray(rflags, np.uint8), (n,)).copy()
    if fixed is not None:
        stride, base = fixed
        buf = np.random.default_rng(77).integers(0, 256, base + n * stride + 64, dtype=np.uint8)
        offs = base + np.arange(n, dtype=np.uint64) * stride
        for o, r in zip(offs, recs):
            assert len(r) <= stride
            buf[int(o):int(o) + len(r)] = np.frombuffer(r, np.uint8)
        lens = np.full(n, stride, np.uint32)
    else:
        buf, offs, lens = P.pack(recs, gap_rng=np.random.default_rng(gap_seed))
    desc = E.make_descriptors(offs, lens, kinds_a, flags_a)
    oracle.batch_emit(buf, desc, n)
    for i, o in zero:
        buf[int(offs[i]) + o:int(offs[i]) + o + 2] = 0
    for i, o, bit in flips:
        buf[int(offs[i]) + o] ^= 1 << bit
    placed = [bytes(buf[int(o):int(o) + int(ln)]) for o, ln in zip(offs, lens)]
    ref_st = oracle.batch_verify(buf.copy(), desc, n, caps=caps)
    sk, arena_size, meta_size = socks.socks()
    assert len(sk) == len(groups)
    exp = R.expected(placed, kinds_a, flags_a, groups, sk, ref_st, arena_size, meta_size)
    exp["status"] = ref_st
    return buf, offs, lens, kinds_a, flags_a, groups, sk, exp


def _run(eng, recs, groups, socks, kinds=E.KIND_ETH, rflags=0, caps=NOCAPS, fixed=None, flips=(), zero=(), gap_seed=1, blocks=0,
         stream=None, graph=False):
    """One verify_udp_enqueue call, compared exactly (the comparisons of the module docstring).  recs: the
    frames; groups: (first, count) or (first, count, reserved) each; socks: a Socks, one row per group; flips:
    (record, byte offset, bit) corrupt single bits after the oracle's emit has filled every checksum; zero:
    (record, byte offset) of 16-bit fields set to 0 after it; fixed: (stride, base) for a fixed-stride batch;
    graph: capture the call on a side stream and replay the graph.  Returns the model's dict plus "status" and
    "got_arena"."""
    buf, offs, lens, kinds_a, flags_a, groups, sk, exp = _model(recs, groups, socks, kinds, rflags, caps, fixed, flips, zero,
                                                               gap_seed)
    n, ref_st, arena_size, meta_size = len(recs), exp["status"], exp["arena"].size, exp["meta"].size
    written = exp["written"]
    want_st = np.where(written, ref_st, PRE).astype(np.uint8)
    want_rx = exp["rx"].view(np.uint8).reshape(n, 16).copy()
    want_rx[~written] = PRE
    want_meta = exp["meta"].view(np.uint8).reshape(meta_size, 48).copy()
    want_meta[~exp["meta_written"]] = PRE

    eng.set_max_blocks(blocks)
    try:
        d = torch.from_numpy(buf.copy()).cuda()
        if fixed is not None:
            batch = E.Batch.fixed(n, fixed[0], fixed[0], int(kinds_a[0]), flags=int(flags_a[0]))
            dv = d[fixed[1]:]
        else:
            batch = E.Batch.from_records(offs, lens, kinds_a, "cuda:0", flags=flags_a)
            dv = d
        gh = E.make_groups([g[0] for g in groups], [g[1] for g in groups])
        gh["reserved"] = [g[2] for g in groups]
        gd = torch.from_numpy(gh.view(np.uint8).copy()).cuda()
        sd = torch.from_numpy(sk.view(np.uint8).copy()).cuda()
        dst = torch.full((arena_size,), R.SENTINEL, dtype=torch.uint8, device="cuda")
        md = torch.full((meta_size, 48), PRE, dtype=torch.uint8, device="cuda")
        st0 = torch.full((n,), PRE, dtype=torch.uint8, device="cuda")
        rx0 = torch.full((n, 16), PRE, dtype=torch.uint8, device="cuda")
        out0 = torch.full((len(groups), 32), PRE, dtype=torch.uint8, device="cuda")
        call = lambda s: eng.verify_udp_enqueue(dv, batch, gd, dst, sd, md, caps=caps, status=st0, rx=rx0, out=out0, stream=s)
        if graph:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                call(side)  # (warm-up outside the capture)
                side.synchronize()
                dst.fill_(R.SENTINEL), md.fill_(PRE), st0.fill_(PRE), rx0.fill_(PRE), out0.fill_(PRE)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=side):
                    call(side)
                side.synchronize()
                assert bool((dst == R.SENTINEL).all()) and bool((st0 == PRE).all()), "the capture itself ran the kernel"
                g.replay()
                side.synchronize()
        elif stream is not None:
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                call(stream)
            stream.synchronize()
        else:
            call(None)
        launched = eng.last_launch()
        vst = eng.verify(dv, batch, caps=caps)
        got_st, got_vst, got_dst = st0.cpu().numpy(), vst.cpu().numpy(), dst.cpu().numpy()
        got_rx, got_meta = rx0.cpu().numpy().reshape(n, 16), md.cpu().numpy()
        got_out = out0.cpu().numpy().reshape(-1).view(E.UDPSOCKOUT_DTYPE)
        assert np.array_equal(d.cpu().numpy(), buf), "the batch buffer is only read"
    finally:
        eng.set_max_blocks(0)
    assert launched["kernel"] == "udprx_kernel" and launched["G"] == 64, launched
    assert np.array_equal(got_vst, ref_st), "eng.verify differs from the oracle"
    assert np.array_equal(got_st, want_st), np.nonzero(got_st != want_st)[0][:8]
    bad = np.nonzero((got_rx != want_rx).any(axis=1))[0]
    assert bad.size == 0, f"record entries differ at {bad[:8]}: got {got_rx[bad[:4]].view(E.UDPRX_DTYPE)} " \
                          f"want {want_rx[bad[:4]].view(E.UDPRX_DTYPE)}"
    bad = np.nonzero(got_out != exp["outs"])[0]
    assert bad.size == 0, f"group entries differ at {bad[:8]}: got {got_out[bad[:4]]} want {exp['outs'][bad[:4]]}"
    bad = np.nonzero((got_meta != want_meta).any(axis=1))[0]
    assert bad.size == 0, f"metadata entries differ at {bad[:8]}: got {got_meta[bad[:2]].view(E.UDPMETA_DTYPE)} " \
                          f"want {want_meta[bad[:2]].view(E.UDPMETA_DTYPE)}"
    diff = R.check_arena(got_dst, exp)
    assert diff.size == 0, f"ring bytes differ at {diff[:8]} (got {got_dst[diff[:8]]} want {exp['arena'][diff[:8]]})"
    exp["got_arena"] = got_dst
    return exp


def _flags(exp):
    return exp["rx"]["flags"].tolist()


# ---- the rule ----

def test_rule_cases(eng):
    """One group per rule case, rings back to back: the clear of an empty ring with payload_read != 0; an exact
    fit to the ring's end; contig < size <= window - contig (padding); window - contig < size (Full);
    size > payload_cap; the metadata ring full at the start; the metadata ring filled by the padding entry
    (PADDED and FULL together); a metadata ring that wraps; a zero-length datagram; payload_cap == 0."""
    recs, groups, socks = [], [], Socks()

    def case(sizes, seed, **kw):
        first = len(recs)
        recs.extend(dgram(p) for p in rnd(seed, *sizes))
        groups.append((first, len(sizes)))
        socks.add(**kw)

    case([7], 1, P_=32, M=4, pr=19)                              # 0: the clear: ring_off 0
    case([9, 13], 2, P_=40, M=4, pr=10, pl=8)                    # 1, 2: 9 at 18; 13 fits exactly to the end (27..40)
    case([11], 3, P_=40, M=4, pr=12, pl=20)                      # 3: contig 8 < 11 <= 12: padding, then at 0
    case([11], 4, P_=40, M=4, pr=10, pl=20)                      # 4: contig 10, window - contig 10 < 11: Full
    case([41, 40], 5, P_=40, M=4)                                # 5, 6: size > payload_cap; size == payload_cap
    case([5], 6, P_=40, M=3, mr=1, ml=3)                         # 7: metadata full at the start
    case([11, 3], 7, P_=40, M=3, pr=12, pl=20, mr=2, ml=2)       # 8, 9: the padding takes the last entry: PADDED | FULL
    case([4, 5, 6], 8, P_=64, M=4, mr=3, ml=1)                   # 10-12: metadata indices 0, 1, 2 after the wrap
    case([0, 3, 0], 9, P_=16, M=4, pr=5, pl=2)                   # 13-15: zero-length datagrams take an entry
    case([0, 1], 10, P_=0, M=2)                                  # 16, 17: payload_cap == 0: 0 bytes fit, 1 does not
    case([17, 0], 11, P_=17, M=2, pr=3)                          # 18, 19: a full ring still takes a zero-length one
    exp = _run(eng, recs, groups, socks)
    rx, outs = exp["rx"], exp["outs"]
    assert _flags(exp) == [UDP | ENQ, UDP | ENQ, UDP | ENQ, UDP | ENQ | PADDED, UDP | FULL, UDP | FULL, UDP | ENQ, UDP | FULL,
                           UDP | FULL | PADDED, UDP | FULL, UDP | ENQ, UDP | ENQ, UDP | ENQ, UDP | ENQ, UDP | ENQ, UDP | ENQ,
                           UDP | ENQ, UDP | FULL, UDP | ENQ, UDP | ENQ]
    assert rx["ring_off"][[0, 1, 2, 3]].tolist() == [0, 18, 27, 0] and rx["meta_idx"][[10, 11, 12]].tolist() == [0, 1, 2]
    assert (outs["payload_read"][0], outs["payload_len"][0]) == (0, 7) and outs["payload_len"][2] == 20 + 8 + 11
    assert outs["meta_len"][6] == 3 and outs["payload_len"][6] == 28 and outs["restored"].sum() == 0
    assert exp["spec_only"].sum() == 0


def test_rule_random_states(eng):
    """Random small rings in random states, 1 to 6 datagrams each of random sizes around the free space; three
    workgroups walk all groups."""
    rng = np.random.default_rng(31)
    recs, groups, socks = [], [], Socks(gap=0)
    for g in range(120):
        P_ = int(rng.integers(0, 200))
        M = int(rng.integers(0, 7))
        pl = int(rng.integers(0, P_ + 1))
        ml = int(rng.integers(0, M + 1))
        first = len(recs)
        for _ in range(int(rng.integers(1, 7))):
            recs.append(dgram(P.rand_bytes(rng, int(rng.integers(0, max(2, (P_ - pl) // 2 + 8))))))
        groups.append((first, len(recs) - first))
        socks.add(P_=P_, M=M, pr=int(rng.integers(0, P_)) if P_ else 0, pl=pl, mr=int(rng.integers(0, M)) if M else 0, ml=ml,
                  gap=int(rng.integers(0, 3)))
    exp = _run(eng, recs, groups, socks, blocks=3)
    fl = exp["rx"]["flags"]
    assert (fl & ENQ).any() and (fl & FULL).any() and (fl & PADDED).any() and ((fl & (PADDED | FULL)) == (PADDED | FULL)).any()


# ---- verdicts ----

def _bad(i, off=43):
    return (i, off, 3)  # a payload bit of an Ethernet / IPv4 / UDP frame


@pytest.mark.parametrize("where", ["middle", "front", "end", "all"])
def test_corrupted_datagram_moves_its_followers(eng, where):
    """A corrupted datagram takes no space: its followers move down and are RESTORED; the ones in front of it
    keep their place and are not."""
    sizes = [100, 37, 1472, 64, 5]
    recs = [dgram(p) for p in rnd(40, *sizes)]
    bad = {"middle": [2], "front": [0], "end": [4], "all": [0, 1, 2, 3, 4]}[where]
    socks = Socks()
    socks.add(P_=4000, M=8, pr=100, pl=50)
    exp = _run(eng, recs, [(0, 5)], socks, flips=[_bad(i) for i in bad])
    want = [UDP if j in bad else UDP | ENQ | (REST if j > bad[0] else 0) for j in range(5)]
    assert _flags(exp) == want
    assert int(exp["outs"][0]["enqueued"]) == 5 - len(bad) and int(exp["outs"][0]["restored"]) == sum(1 for w in want if w & REST)
    if where == "all":
        assert tuple(exp["outs"][0])[:4] == (100, 50, 0, 0) and not exp["meta_written"].any()


def test_absent_datagram_lets_a_later_one_fit(eng):
    """The speculative layout drops the last datagram (Full); without the corrupted one it fits: it was not
    stored in step 1 and is RESTORED.  The same with the metadata ring as the limit."""
    a, b, c = rnd(41, 60, 50, 40)
    socks = Socks()
    socks.add(P_=128, M=8)          # 60 + 50 + 40 > 128; 60 + 40 fits
    socks.add(P_=1000, M=2)         # two entries: the third datagram only fits without the second
    exp = _run(eng, [dgram(a), dgram(b), dgram(c)] * 2, [(0, 3), (3, 3)], socks, flips=[_bad(1), _bad(4)])
    assert _flags(exp) == [UDP | ENQ, UDP, UDP | ENQ | REST] * 2
    assert exp["rx"]["ring_off"].tolist() == [0, 0, 60] * 2
    # with the UDP checksum not verified on receive the corrupted ones are accepted: the layouts are equal
    for caps in ((0, 3, 0, 0, 0), (0, 2, 0, 0, 0)):
        exp = _run(eng, [dgram(a), dgram(b), dgram(c)] * 2, [(0, 3), (3, 3)], socks, flips=[_bad(1), _bad(4)], caps=caps)
        assert _flags(exp) == [UDP | ENQ, UDP | ENQ, UDP | FULL] * 2 and exp["spec_only"].sum() == 0


def test_absent_datagram_removes_a_padding_entry(eng):
    """Speculatively the third datagram wraps behind a padding entry; without the corrupted second one it fits
    before the ring's end: no padding entry is written, and the record moves (RESTORED)."""
    a, b, c, d = rnd(42, 30, 40, 50, 10)
    socks = Socks()
    socks.add(P_=128, M=8, pr=100, pl=20)  # write index 120 -> clear? no: pl != 0; window 108, contig 8
    socks.add(P_=128, M=8, pr=20, pl=10)   # write index 30: 30 @30, 40 @60, 50: contig 28 -> padding, @0 (window 48 - 28 < 50: Full)
    socks.add(P_=200, M=8, pr=70, pl=10)   # write index 80: 30 @80, 40 @110, 50 @150 fits exactly; no padding either way
    socks.add(P_=160, M=8, pr=60, pl=0)    # cleared: 30 @0, 40 @30, 50 @70, 10 @120
    socks.add(P_=150, M=8, pr=140, pl=5)   # write index 145: 30 pads 5 -> @0, 40 @30, 50 @70; without b: 50 @30
    recs = [dgram(x) for x in (a, b, c, d)] * 5
    groups = [(4 * g, 4) for g in range(5)]
    exp = _run(eng, recs, groups, socks, flips=[_bad(4 * g + 1) for g in range(5)])
    fl = exp["rx"]["flags"].reshape(5, 4)
    assert (fl[:, 1] == UDP).all() and (fl[[2, 3, 4], 2] == UDP | ENQ | REST).all()
    # group 1: speculatively 50 is Full (padding + 28 short); accepted 50 @60 fits before the end: no PADDED
    exp2 = _run(eng, [dgram(a), dgram(b), dgram(c)], [(0, 3)], _one(P_=128, M=8, pr=16, pl=10), flips=[_bad(1)])
    # write index 26: a @26, b @56, c: contig 32 < 50 -> padding, @0 needs 50 <= 118 - 70 - 32: Full;  accepted: c @56
    assert _flags(exp2) == [UDP | ENQ, UDP, UDP | ENQ | REST] and exp2["rx"]["ring_off"].tolist() == [26, 0, 56]
    exp3 = _run(eng, [dgram(a), dgram(b), dgram(c)], [(0, 3)], _one(P_=128, M=8, pr=96, pl=2), flips=[_bad(1)])
    # write index 98: a @98 (to 128), the write index wraps to 0 by itself: b @0, c @40;  accepted: c @0, no padding anywhere
    assert exp3["rx"]["ring_off"].tolist() == [98, 0, 0]
    exp4 = _run(eng, [dgram(b), dgram(a), dgram(c)], [(0, 3)], _one(P_=128, M=8, pr=70, pl=10), flips=[_bad(0)])
    # write index 80: speculatively b @80, a: contig 8 -> PADDING(8), @0, c @30;  accepted: a @80, c: contig 18 -> PADDING(18), @0
    assert _flags(exp4) == [UDP, UDP | ENQ | REST, UDP | ENQ | REST | PADDED] and exp4["rx"]["ring_off"].tolist() == [0, 80, 0]
    exp5 = _run(eng, [dgram(b), dgram(a), dgram(d)], [(0, 3)], _one(P_=128, M=8, pr=70, pl=10), flips=[_bad(0)])
    # speculatively a sits behind PADDING(8) at 0, d @30;  accepted: a @80, d @110: the padding entry is gone
    assert _flags(exp5) == [UDP, UDP | ENQ | REST, UDP | ENQ | REST] and exp5["rx"]["ring_off"].tolist() == [0, 80, 110]
    assert int(exp5["outs"][0]["meta_len"]) == 2 and exp5["meta_written"].sum() == 2


def _one(**kw):
    s = Socks()
    s.add(**kw)
    return s


# ---- parsing and caps ----

def test_parsing_forms(eng):
    """IPv6, IPv4 options, a Hop-by-Hop header (a short one, and a long one that pushes the UDP header out of the
    128-byte window), Ethernet padding (not delivered), a UDP / IPv4 zero checksum field (accepted), in one
    group; then the same as IP records without Ethernet."""
    rng = np.random.default_rng(43)
    p = rnd(43, 33, 17, 100, 61, 5, 29, 1)
    recs = [
        dgram(p[0], v6=True),
        dgram(p[1], options=bytes([1, 1, 1, 1, 1, 1, 1, 0])),
        dgram(p[2], v6=True, hbh=P.hbh(17, 0, rng)),
        dgram(p[3], v6=True, hbh=P.hbh(17, 14, rng)),
        dgram(p[4], pad=13),
        dgram(p[5]),
        dgram(p[6], v6=True, pad=3, sport=1),
    ]
    zero = [(5, 14 + 20 + 6)]
    exp = _run(eng, recs, [(0, 7)], _one(P_=512, M=8, pr=500, pl=3), zero=zero)
    assert _flags(exp)[1:] == [UDP | ENQ] * 6 and _flags(exp)[0] == UDP | ENQ | PADDED and (exp["status"] & E.ST_ACCEPT).all()
    assert exp["rx"]["len"].tolist() == [33, 17, 100, 61, 5, 29, 1]
    assert exp["meta"]["family"][exp["meta_written"]].tolist() == [0, 6, 4, 6, 6, 4, 4, 6]
    exp = _run(eng, [r[14:] for r in recs], [(0, 7)], _one(P_=512, M=8), kinds=E.KIND_IP, zero=[(5, 20 + 6)])
    assert _flags(exp) == [UDP | ENQ] * 7


@pytest.mark.parametrize("udp_caps", [0, 1, 2, 3])
@pytest.mark.parametrize("ip_caps", [0, 1, 2, 3])
def test_caps_receive_settings(eng, udp_caps, ip_caps):
    """Every receive setting of caps.udp and caps.ipv4 over one group with a bad UDP checksum, a bad IPv4 header
    checksum, a good datagram and a bad UDP / IPv6 checksum: who takes space follows the status byte."""
    a, b, c, d = rnd(44, 40, 41, 42, 43)
    recs = [dgram(a), dgram(b), dgram(c), dgram(d, v6=True)]
    exp = _run(eng, recs, [(0, 4)], _one(P_=100, M=8), caps=(ip_caps, udp_caps, 0, 0, 0),
               flips=[(0, 50, 2), (1, 14 + 8, 1), (3, 14 + 40 + 8 + 11, 6)])
    udp_rx, ip_rx = udp_caps in (0, 1), ip_caps in (0, 1)
    acc = [not udp_rx, not ip_rx, True, not udp_rx]
    assert ((exp["status"] & E.ST_ACCEPT) != 0).tolist() == acc
    assert [bool(f & (ENQ | FULL)) for f in _flags(exp)] == acc


# ---- groups and batches ----

def test_mixed_groups(eng):
    """Groups that mix in TCP, ICMP, an IPv4 fragment, a malformed record (UDP length past the packet), a UDP
    datagram to port 0, a non-IP ethertype and a port mismatch; a second socket bound to the other port takes
    what the first one leaves out; raw and header-only records have no candidates."""
    p = rnd(45, 20, 21, 22, 23, 24, 25, 26, 27)
    recs = [
        dgram(p[0]),
        P.eth(P.ipv4(A4, B4, 6, P.tcp(1000, PORT, p[1]))),
        P.eth(P.ipv4(A4, B4, 1, P.icmp_echo(8, p[2]))),
        dgram(p[3], dport=PORT + 1),
        P.eth(P.ipv4(A4, B4, 17, P.udp(7, PORT, p[4]), flags_frag=0x2000)),
        P.eth(P.ipv4(A4, B4, 17, P.udp(7, PORT, p[5], length=8 + 26))),
        dgram(p[6], dport=0),
        P.eth(p[7] + bytes(40), 0x0806),
        dgram(p[1]),
    ]
    socks = Socks()
    socks.add(P_=64, M=4)
    socks.add(P_=64, M=4, port=PORT + 1)
    exp = _run(eng, recs * 2, [(0, 9), (9, 9)], socks)
    assert _flags(exp) == [UDP | ENQ] + [0] * 7 + [UDP | ENQ] + [0] * 3 + [UDP | ENQ] + [0] * 5
    ip = [r[14:] for i, r in enumerate(recs) if i != 7]
    exp = _run(eng, ip, [(0, 8)], _one(P_=64, M=4), kinds=E.KIND_RAW)
    assert not any(_flags(exp)) and int(exp["outs"][0]["valid"]) == 1
    exp = _run(eng, ip, [(0, 8)], _one(P_=64, M=4), kinds=E.KIND_IP, rflags=E.REC_IPHDR_ONLY)
    assert not any(_flags(exp))


def test_fixed_stride_batch(eng):
    """The implicit batch form: frames at a fixed stride from an odd base, each record longer than its frame."""
    p = rnd(46, 1472, 700, 1, 1472, 333)
    recs = [dgram(x) for x in p]
    socks = Socks()
    socks.add(P_=4096, M=8, pr=4000, pl=0)
    socks.add(P_=1805, M=2, pr=5, pl=0)
    exp = _run(eng, recs, [(0, 3), (3, 2)], socks, fixed=(1531, 7))
    assert _flags(exp) == [UDP | ENQ] * 5 and exp["rx"]["ring_off"].tolist() == [0, 1472, 2172, 0, 1472]


def test_jumbo_frame_and_256_records(eng):
    """One 9000-byte frame (several steps of 1024 bytes) behind a short one; a group of 256 datagrams, the most
    a group holds, five of them corrupted, into a ring that wraps once and a metadata ring that wraps."""
    rng = np.random.default_rng(47)
    recs = [dgram(P.rand_bytes(rng, 11)), dgram(P.rand_bytes(rng, 9000 - 42))]
    recs += [dgram(P.rand_bytes(rng, 20 + j % 7)) for j in range(256)]
    socks = Socks()
    socks.add(P_=9100, M=4, pr=17, pl=1)
    socks.add(P_=8000, M=300, pr=4000, pl=100, mr=290, ml=3)
    exp = _run(eng, recs, [(0, 2), (2, 256)], socks, flips=[_bad(2 + j) for j in range(10, 256, 50)])
    assert _flags(exp)[:2] == [UDP | ENQ, UDP | ENQ] and int(exp["outs"][1]["enqueued"]) == 251
    assert int(exp["outs"][1]["restored"]) >= 200 and ((exp["rx"]["flags"][2:] & PADDED) != 0).sum() == 1
    assert (exp["rx"]["flags"][2:12] == UDP | ENQ).all()


def test_invalid_groups_and_records_outside_groups(eng):
    """Invalid groups (outside the batch, count 0 or 257, reserved words of the group or the socket entry, a ring
    fuller than its capacity, a read index outside its ring) write a zero group entry and nothing else; records
    outside every group keep their status byte and entry."""
    rng = np.random.default_rng(48)
    n = 300
    recs = [dgram(P.rand_bytes(rng, 10)) for _ in range(n)]
    socks, groups = Socks(gap=2), []

    def add(g, **kw):
        groups.append(g)
        socks.add(**{**dict(P_=64, M=4), **kw})

    add((0, 2))
    add((n, 1))
    add((n - 1, 2))
    add((4, 0))
    add((5, 257))
    add((5, 1, 7))
    add((6, 1), reserved=(1, 0, 0))
    add((7, 1), reserved=(0, 0, 2))
    add((8, 1), pl=65)
    add((9, 1), ml=5)
    add((10, 1), pr=64)
    add((11, 1), mr=4)
    add((12, 1), P_=0, pr=1)
    add((13, 1), M=0, mr=1)
    add((14, 1), P_=0, M=0)
    add((15, 2))
    add((40, 256), P_=4000, M=256)
    exp = _run(eng, recs, groups, socks)
    assert exp["outs"]["valid"].tolist() == [1] + [0] * 13 + [1, 1, 1]
    assert int(exp["outs"][16]["enqueued"]) == 256 and _flags(exp)[14] == UDP | FULL


# ---- placement ----

def test_odd_lengths_at_odd_offsets_back_to_back(eng):
    """Odd payload lengths at every ring offset mod 16 and every source alignment, rings of different groups back
    to back (and one byte apart): a neighbour's bytes stay intact, since the whole arena is compared."""
    rng = np.random.default_rng(49)
    recs, groups, socks = [], [], Socks(start=1, gap=0)
    for g in range(48):
        sizes = [int(rng.choice([1, 3, 15, 17, 31, 33, 47, 99])) for _ in range(3)]
        first = len(recs)
        recs.extend(dgram(P.rand_bytes(rng, s), v6=bool(g & 1)) for s in sizes)
        groups.append((first, 3))
        start = g % 16
        socks.add(P_=start + sum(sizes) + g % 3, M=3, pr=0, pl=start, gap=g % 2)
    for seed in range(3):
        exp = _run(eng, recs, groups, socks, gap_seed=seed)
        assert (exp["rx"]["flags"] == UDP | ENQ).all()


def test_equal_layouts_write_nothing_outside_the_enqueued_ranges(eng):
    """Every candidate accepted: the speculative and the accepted layout are equal, nothing is RESTORED, and the
    arena shows the sentinel at every byte outside the ENQUEUED ranges (padding and occupied bytes included)."""
    recs = [dgram(x) for x in rnd(50, 300, 200, 90, 150)]
    exp = _run(eng, recs, [(0, 4)], _one(P_=700, M=8, pr=100, pl=50))  # 300 @150, 200 @450, 90: PADDING(50) @0, 150 Full
    assert _flags(exp) == [UDP | ENQ, UDP | ENQ, UDP | ENQ | PADDED, UDP | FULL] and exp["spec_only"].sum() == 0
    got = exp["got_arena"]
    inside = np.zeros(got.size, bool)
    for e in exp["rx"][:3]:
        inside[3 + int(e["ring_off"]):3 + int(e["ring_off"]) + int(e["len"])] = True
    assert inside.sum() == 590 and (got[~inside] == R.SENTINEL).all()


def test_graph_capture_and_replay_on_a_side_stream(eng):
    """The call is captured into a graph on a side stream (no allocation, no event, no host synchronisation) and
    the replay does the work, the restore pass included."""
    recs = [dgram(x) for x in rnd(51, 100, 200, 300, 17)]
    socks = Socks()
    socks.add(P_=1000, M=8, pr=900, pl=20)
    socks.add(P_=1000, M=8)
    exp = _run(eng, recs * 2, [(0, 4), (4, 4)], socks, flips=[_bad(1)], graph=True)
    assert exp["outs"]["restored"].tolist() == [2, 0]


def test_stream_and_empty_call(eng):
    """A non-default stream; n_groups == 0 launches nothing and writes nothing."""
    recs = [dgram(x) for x in rnd(52, 200, 200)]
    _run(eng, recs, [(0, 2)], _one(P_=400, M=2), stream=torch.cuda.Stream())
    d = torch.zeros(256, dtype=torch.uint8, device="cuda")
    dst = torch.full((64,), R.SENTINEL, dtype=torch.uint8, device="cuda")
    md = torch.full((4, 48), PRE, dtype=torch.uint8, device="cuda")
    empty = torch.zeros(0, dtype=torch.uint8, device="cuda")
    eng.verify(d, E.Batch.fixed(4, 64, 64, E.KIND_IP))
    st, rx, out = eng.verify_udp_enqueue(d, E.Batch.fixed(4, 64, 64, E.KIND_IP), empty, dst, empty, md,
                                         status=torch.full((4,), PRE, dtype=torch.uint8, device="cuda"))
    assert eng.last_launch()["kernel"] != "udprx_kernel"
    assert bool((st == PRE).all()) and bool((dst == R.SENTINEL).all()) and bool((md == PRE).all()) and out.numel() == 0
