"""GPU parity of verify_tcp_assemble (smol_csum_batch_verify_tcp_assemble): verify's status bytes, one
smol_csum_tcpseg_t per record, one smol_csum_tcpflow_t per group, and every TCP segment's payload put at
its sequence number's place in its connection's receive ring, trimmed to the window, in one pass.

Every case compares exactly:
  1. the status bytes with oracle.batch_verify, and with eng.verify on the same batch;
  2. the segment and flow entries with tests/tcp_assemble_ref.py;
  3. the WHOLE destination arena, filled with the sentinel 0xA5 beforehand, with the helper's: a stray
     store or a missing byte anywhere fails;
  4. the batch buffer: it is only read;
and asserts that the launch was tcpasm_kernel.  Status bytes and segment entries of records the call must
not write keep their fill.

Overlapping records of one flow carry slices of one byte stream, so their bytes agree wherever the contract
leaves the winner open; a corrupted copy differs from its retransmission only where a counted record covers
it."""
import numpy as np
import pytest

import oracle
from tests import pktgen as P
from tests import tcp_assemble_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from smoltcp_amd import engine as E  # noqa: E402

NOCAPS = (0, 0, 0, 0, 0)
PRE = 0x5A  # the fill of the status and segment tensors: bytes the call must not write keep it
A4, B4 = bytes([10, 1, 2, 3]), bytes([10, 4, 5, 6])
A6, B6 = bytes(range(0x20, 0x30)), bytes(range(0x40, 0x50))


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    e = E.ChecksumEngine(0)
    yield e
    e.close()


def frame(seq, payload, flags=0x18, doff=5, v6=False, eth=True, pad=0, sport=1000, dport=80):
    """One TCP frame (checksums 0: the oracle's emit fills them); pad: Ethernet padding after the IP packet."""
    seg = P.tcp(sport, dport, payload, seq=seq & 0xFFFFFFFF, flags=flags, doff=doff)
    ip = P.ipv6(A6, B6, 6, seg) if v6 else P.ipv4(A4, B4, 6, seg)
    return (P.eth(ip, 0x86DD if v6 else 0x0800) if eth else ip) + bytes(pad)


class Rings:
    """Rings laid out one after the other in the arena, 0..20 bytes between them, each start at any alignment."""

    def __init__(self, seed=0, start=3):
        self.rng, self.pos, self.rows = np.random.default_rng(seed), start, []

    def add(self, window_start, window_len, ring_len=None, ring_pos=None, reserved=(0, 0), dst_mod=None):
        ring_len = window_len if ring_len is None else ring_len
        self.pos += int(self.rng.integers(0, 21))
        if dst_mod is not None:
            self.pos += (dst_mod - self.pos) % 16
        if ring_pos is None:
            ring_pos = int(self.rng.integers(0, ring_len)) if ring_len else 0
        self.rows.append((self.pos, ring_len, ring_pos, window_start & 0xFFFFFFFF, window_len, reserved))
        self.pos += ring_len
        return len(self.rows) - 1

    def wins(self):
        w = E.make_tcpwins(*[[r[i] for r in self.rows] for i in range(5)])
        w["reserved"] = [r[5] for r in self.rows]
        return w, self.pos + 19


def _run(eng, recs, groups, rings, kinds=E.KIND_ETH, rflags=0, caps=NOCAPS, fixed=None, flips=(), gap_seed=1, blocks=0,
         stream=None):
    """One verify_tcp_assemble call, compared exactly (the comparisons of the module docstring).  recs: the
    frames; groups: (first, count) or (first, count, reserved) each; rings: a Rings, one row per group; flips:
    (record, byte offset, bit) corrupt single bits after the oracle's emit has filled every checksum; fixed:
    (stride, base) for a fixed-stride batch.  Returns (status, segs, flows) as numpy arrays."""
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
    for i, o, bit in flips:
        buf[int(offs[i]) + o] ^= 1 << bit
    placed = [bytes(buf[int(o):int(o) + int(ln)]) for o, ln in zip(offs, lens)]
    ref_st = oracle.batch_verify(buf.copy(), desc, n, caps=caps)
    wins, arena_size = rings.wins()
    assert len(wins) == len(groups)
    ref_segs, ref_flows, ref_arena, written = R.expected(placed, kinds_a, flags_a, groups, wins, (ref_st & E.ST_ACCEPT) != 0,
                                                         arena_size)
    want_st = np.where(written, ref_st, PRE).astype(np.uint8)
    want_segs = ref_segs.view(np.uint8).reshape(n, 16).copy()
    want_segs[~written] = PRE

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
        wd = torch.from_numpy(wins.view(np.uint8).copy()).cuda()
        dst = torch.full((arena_size,), R.SENTINEL, dtype=torch.uint8, device="cuda")
        st0 = torch.full((n,), PRE, dtype=torch.uint8, device="cuda")
        sg0 = torch.full((n, 16), PRE, dtype=torch.uint8, device="cuda")
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                st, sg, fl = eng.verify_tcp_assemble(dv, batch, gd, dst, wd, caps=caps, status=st0, segs=sg0, stream=stream)
            stream.synchronize()
        else:
            st, sg, fl = eng.verify_tcp_assemble(dv, batch, gd, dst, wd, caps=caps, status=st0, segs=sg0)
        launched = eng.last_launch()
        vst = eng.verify(dv, batch, caps=caps)
        got_st, got_vst, got_dst = st.cpu().numpy(), vst.cpu().numpy(), dst.cpu().numpy()
        got_sg = sg.cpu().numpy().reshape(n, 16)
        got_fl = fl.cpu().numpy().reshape(-1).view(E.TCPFLOW_DTYPE)
        assert np.array_equal(d.cpu().numpy(), buf), "the batch buffer is only read"
    finally:
        eng.set_max_blocks(0)
    assert launched["kernel"] == "tcpasm_kernel" and launched["G"] == 64, launched
    assert np.array_equal(got_vst, ref_st), "eng.verify differs from the oracle"
    assert np.array_equal(got_st, want_st), np.nonzero(got_st != want_st)[0][:8]
    assert np.array_equal(got_st[written], got_vst[written])
    bad = np.nonzero((got_sg != want_segs).any(axis=1))[0]
    assert bad.size == 0, f"segment entries differ at {bad[:8]}: got {got_sg[bad[:4]].view(E.TCPSEG_DTYPE)} " \
                          f"want {want_segs[bad[:4]].view(E.TCPSEG_DTYPE)}"
    bad = np.nonzero(got_fl != ref_flows)[0]
    assert bad.size == 0, f"flow entries differ at {bad[:8]}: got {got_fl[bad[:4]]} want {ref_flows[bad[:4]]}"
    diff = np.nonzero(got_dst != ref_arena)[0]
    assert diff.size == 0, f"ring bytes differ at {diff[:8]} (got {got_dst[diff[:8]]} want {ref_arena[diff[:8]]})"
    return ref_st, ref_segs, ref_flows


def test_window_rule_sweep(eng):
    """One-record flows: W in {0, 1, 7, 64}, p in {0, 1, 5, 16, 17}, s from -(p + 1) to W + 1, window_start
    near 2^32 so that seq wraps; rings a little larger than the window at random positions."""
    rng = np.random.default_rng(11)
    recs, groups, rings = [], [], Rings(1)
    for W in (0, 1, 7, 64):
        for p in (0, 1, 5, 16, 17):
            for s in range(-(p + 1), W + 2):
                ws = 0xFFFFFFF0 + len(recs) % 32
                recs.append(frame(ws + s, P.rand_bytes(rng, p)))
                groups.append((len(recs) - 1, 1))
                rings.add(ws, W, ring_len=W + len(recs) % 3)
    _, segs, flows = _run(eng, recs, groups, rings)
    inw = (segs["flags"] & R.SEG_IN_WINDOW) != 0
    assert inw.any() and (~inw).any() and (flows["contig_len"] > 0).any() and (segs["len"][inw] == 0).any()


def test_ring_wrap_at_every_position_and_alignment(eng):
    """100-byte payloads into 160-byte rings at every ring position: the range wraps from position 61 on, a
    piece ends exactly at the ring's end at 60; every destination alignment; random source alignments."""
    rng = np.random.default_rng(12)
    recs, groups, rings = [], [], Rings(2)
    for pos in range(160):
        recs.append(frame(5000 + 3, P.rand_bytes(rng, 97)))
        groups.append((pos, 1))
        rings.add(5000, 120, ring_len=160, ring_pos=(pos + 160 - 3) % 160, dst_mod=pos % 16)
    _run(eng, recs, groups, rings)


@pytest.mark.parametrize("count,pay", [(1, 1460), (2, 1460), (3, 700), (4, 1460), (5, 33), (7, 1460), (45, 1460), (64, 100),
                                       (255, 40), (256, 24)])
def test_in_order_flows(eng, count, pay):
    """Flows of `count` in-order segments (record j to wave j mod 4; 256: the most a group holds), the front
    of the ring holding the stream; a second flow of the same size shuffled."""
    rng = np.random.default_rng(count)
    total = count * pay
    stream = P.rand_bytes(rng, total)
    recs = [frame(77 + j * pay, stream[j * pay:(j + 1) * pay]) for j in range(count)]
    order = rng.permutation(count)
    recs += [frame(0x7FFFFF00 + int(j) * pay, stream[int(j) * pay:(int(j) + 1) * pay]) for j in order]
    rings = Rings(3)
    rings.add(77, total, ring_len=total + 5)
    rings.add(0x7FFFFF00, total, ring_len=total)
    _, segs, flows = _run(eng, recs, [(0, count), (count, count)], rings)
    assert flows["contig_len"].tolist() == [total, total] and flows["counted"].tolist() == [count, count]


def test_holes_duplicates_and_trims(eng):
    """Random flows of slices of one stream: holes, duplicates, overlaps, segments reaching in front of the
    window and past its end, empty segments; several workgroups' worth of groups on three workgroups, so
    each walks many groups."""
    rng = np.random.default_rng(14)
    recs, groups, rings = [], [], Rings(4)
    for g in range(40):
        W = int(rng.integers(1, 3000))
        ws = int(rng.choice([9, 0xFFFFFC00, 0x7FFFFE00, int(rng.integers(0, 1 << 32))]))
        before = 200
        stream = P.rand_bytes(rng, before + W + 200)
        first = len(recs)
        for _ in range(int(rng.integers(1, 12))):
            a = int(rng.integers(-before, W + 50))
            b = min(a + int(rng.integers(0, 900)), W + 200)
            recs.append(frame(ws + a, stream[before + a:before + max(a, b)], doff=int(rng.choice([5, 8, 15]))))
        groups.append((first, len(recs) - first))
        rings.add(ws, W, ring_len=W + int(rng.integers(0, 40)))
    _, segs, flows = _run(eng, recs, groups, rings, blocks=3)
    assert (flows["contig_len"] > 0).any() and (flows["contig_len"] == 0).any()
    assert ((segs["flags"] & R.SEG_IN_WINDOW) == 0).any()


def test_corrupted_segments_and_retransmissions(eng):
    """A corrupted segment and its retransmission in one poll, in both arrival orders, partly overlapping and
    wrapping: the ring holds the good bytes, the good copy is REDELIVERED.  A corrupted segment alone stays in
    the ring and counts for nothing.  With the TCP checksum not verified (caps), the same records all count."""
    rng = np.random.default_rng(15)
    data = P.rand_bytes(rng, 4000)
    seg = lambda ws, a, b: frame(ws + a, data[a:b])
    recs, groups, rings, flips = [], [], Rings(5), []

    def flow(ws, W, parts, bad, **kw):
        first = len(recs)
        for j, (a, b) in enumerate(parts):
            recs.append(seg(ws, a, b))
            if j in bad:
                flips.append((len(recs) - 1, 54 + (b - a) // 2, 3))  # a payload bit
        groups.append((first, len(parts)))
        rings.add(ws, W, **kw)

    flow(100, 3000, [(0, 1460), (0, 1460), (1460, 2920)], {0})                      # bad copy first
    flow(200, 3000, [(0, 1460), (1460, 2920), (0, 1460)], {2})                      # bad copy last
    flow(300, 3000, [(500, 1500), (0, 700), (700, 1300), (1300, 2000)], {0})        # a bad one under three good ones
    flow(400, 3000, [(0, 1000), (1000, 2000)], {1})                                 # a bad one alone: a hole for the caller
    flow(500, 2000, [(0, 1460), (0, 1460)], {1}, ring_len=2000, ring_pos=1200)      # wrapping
    flow(600, 3000, [(j * 100, j * 100 + 100) for j in range(20)] + [(0, 2000)], {20})  # one bad under twenty good
    flow(700, 3000, [(0, 100), (100, 200)], {0, 1})                                  # nothing counts
    st, segs, flows = _run(eng, recs, groups, rings, flips=flips)
    assert flows["redelivered"].tolist() == [1, 1, 3, 0, 1, 20, 0]
    assert flows["contig_len"].tolist() == [2920, 2920, 2000, 1000, 1460, 2000, 0]
    assert flows["counted"].tolist() == [2, 2, 3, 1, 1, 20, 0]
    # the same records with the checksum field itself corrupted, so that the payloads agree: rejected under the
    # default caps; with the TCP checksum not verified (Checksum::None) every record counts, nothing is redelivered
    field = [(i, 14 + 20 + 16, 3) for i, _, _ in flips]
    st, _, flows = _run(eng, recs, groups, rings, flips=field)
    assert not (st[[i for i, _, _ in flips]] & E.ST_ACCEPT).any() and flows["redelivered"].tolist() == [1, 1, 3, 0, 1, 20, 0]
    st, _, flows = _run(eng, recs, groups, rings, flips=field, caps=(0, 0, 3, 0, 0))
    assert (st & E.ST_ACCEPT).all() and not flows["redelivered"].any()
    assert flows["contig_len"].tolist() == [2920, 2920, 2000, 2000, 1460, 2000, 200]


def test_records_without_a_tcp_span_syn_rst_and_padding(eng):
    """UDP, ICMP, a TCP segment with port 0 (malformed), an IPv4 fragment, IPv6 TCP, a Hop-by-Hop header in
    front of TCP, a long one that pushes the TCP header out of the 128-byte window, SYN, RST, TCP options,
    Ethernet padding after a short segment, a non-IP ethertype: all inside one flow's group."""
    rng = np.random.default_rng(16)
    ws = 0x10000000
    data = P.rand_bytes(rng, 2000)
    d = lambda a, b: data[a:b]
    hbh = lambda units: P.hbh(6, units, rng)
    recs = [
        frame(ws, d(0, 100)),
        P.eth(P.ipv4(A4, B4, 17, P.udp(7, 9, d(0, 50)))),
        P.eth(P.ipv4(A4, B4, 1, P.icmp_echo(8, d(0, 40)))),
        frame(ws + 100, d(100, 200), dport=0),
        P.eth(P.ipv4(A4, B4, 6, P.tcp(1000, 80, d(100, 200), seq=ws + 100), flags_frag=0x2000)),
        frame(ws + 100, d(100, 300), v6=True),
        P.eth(P.ipv6(A6, B6, 0, hbh(0) + P.tcp(1000, 80, d(300, 400), seq=ws + 300)), 0x86DD),
        P.eth(P.ipv6(A6, B6, 0, hbh(14) + P.tcp(1000, 80, d(400, 600), seq=ws + 400)), 0x86DD),
        frame(ws + 600, d(600, 610), flags=0x02),
        frame(ws + 600, d(600, 610), flags=0x14),
        frame(ws + 600, d(600, 700), doff=15),
        frame(ws + 700, d(700, 703), pad=17),
        frame(ws + 703, b"", pad=6),
        P.eth(d(0, 64), 0x0806),
        frame(ws + 703, d(703, 2000)),
    ]
    rings = Rings(6)
    rings.add(ws, 1900, ring_len=2048, ring_pos=2000)
    st, segs, flows = _run(eng, recs, [(0, len(recs))], rings)
    assert segs["flags"].tolist() == [7, 0, 0, 0, 0, 7, 7, 7, 3, 3, 7, 7, 7, 0, 7]
    assert int(flows[0]["contig_len"]) == 1900 and int(flows[0]["counted"]) == 7  # (the empty segment delivers nothing)
    # the same as IP records without Ethernet, and as raw records (no span at all)
    ip = [r[14:] for i, r in enumerate(recs) if i != 13]
    rings = Rings(6)
    rings.add(ws, 1900, ring_len=2048, ring_pos=2000)
    _run(eng, ip, [(0, len(ip))], rings, kinds=E.KIND_IP)
    _, segs, flows = _run(eng, ip, [(0, len(ip))], rings, kinds=E.KIND_RAW)
    assert not segs["flags"].any() and int(flows[0]["valid"]) == 1 and int(flows[0]["counted"]) == 0
    _, segs, _ = _run(eng, ip, [(0, len(ip))], rings, kinds=E.KIND_IP, rflags=E.REC_IPHDR_ONLY)
    assert not segs["flags"].any()


def test_long_records_take_several_steps(eng):
    """Payloads past one step of 2048 bytes (jumbo frames), trimmed at the front and the back and wrapping,
    at every source alignment."""
    rng = np.random.default_rng(17)
    before = 2100
    data = P.rand_bytes(rng, before + 9000)  # data[before + o] is the byte at window offset o
    recs, groups, rings = [], [], Rings(7)
    for i, (a, b, W, rl, rp) in enumerate([(0, 4000, 4000, 4000, 0), (-700, 5000, 4100, 4100, 3000), (100, 8900, 6000, 7001, 6990),
                                           (0, 2049, 2049, 2060, 11), (-2100, 2100, 5000, 5000, 4999), (0, 8960, 8960, 8960, 1)]):
        ws = 0xFFFFF000 + i
        recs.append(frame(ws + a, data[before + a:before + b]))
        groups.append((i, 1))
        rings.add(ws, W, ring_len=rl, ring_pos=rp)
    for seed in range(4):
        _run(eng, recs, groups, rings, gap_seed=seed)


def test_fixed_stride_batch(eng):
    """The implicit batch form: frames at a fixed stride from an odd base, each record longer than its frame."""
    rng = np.random.default_rng(18)
    data = P.rand_bytes(rng, 6 * 1460)
    recs = [frame(9 + j * 1460, data[j * 1460:(j + 1) * 1460]) for j in (0, 2, 1, 5, 3)] + [frame(9, data[:10])]
    rings = Rings(8)
    rings.add(9, 8000, ring_len=8192, ring_pos=8000)
    rings.add(9, 5, ring_len=8)
    _, segs, flows = _run(eng, recs, [(0, 5), (5, 1)], rings, fixed=(1531, 7))
    assert flows["contig_len"].tolist() == [4 * 1460, 5]


def test_invalid_groups_and_records_outside_groups(eng):
    """Invalid groups (outside the batch, count 0 or 257, reserved words, a window larger than its ring, a ring
    position outside the ring) write a zero flow entry and nothing else; records outside every group keep their
    status byte and segment entry; a valid ring of length 0."""
    rng = np.random.default_rng(19)
    n = 300
    recs = [frame(50 + 10 * j, P.rand_bytes(rng, 10)) for j in range(n)]
    rings = Rings(9)
    groups = []

    def add(g, W=64, **kw):
        groups.append(g)
        rings.add(50 + 10 * g[0], W, **kw)

    add((0, 2))
    add((n, 1))
    add((n - 1, 2))
    add((4, 0))
    add((5, 257))
    add((5, 1, 7))
    add((6, 1), reserved=(1, 0))
    add((7, 1), reserved=(0, 2))
    add((8, 1), ring_len=63)
    add((9, 1), ring_len=64, ring_pos=64)
    add((10, 1), W=0, ring_len=0, ring_pos=1)
    add((11, 1), W=0, ring_len=0, ring_pos=0)
    add((12, 2))
    add((40, 256), W=4000)
    _, segs, flows = _run(eng, recs, groups, rings)
    assert flows["valid"].tolist() == [1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1]
    assert int(flows[13]["contig_len"]) == 2560 and int(flows[13]["counted"]) == 256


def test_destination_past_4_gib(eng):
    """A ring whose dst_offset does not fit 32 bits: the offset is 64-bit all the way."""
    rng = np.random.default_rng(20)
    data = P.rand_bytes(rng, 3000)
    recs = [frame(1 + j * 1000, data[j * 1000:(j + 1) * 1000]) for j in (1, 0, 2)]
    buf, offs, lens = P.pack(recs, gap_rng=np.random.default_rng(1))
    oracle.batch_emit(buf, E.make_descriptors(offs, lens, E.KIND_ETH), 3)
    base = (1 << 32) + 4093
    size = base + 3000 + 64
    dst = torch.full((size,), R.SENTINEL, dtype=torch.uint8, device="cuda")
    wins = E.make_tcpwins([base], 3000, 2500, 1, 3000)
    d = torch.from_numpy(buf.copy()).cuda()
    batch = E.Batch.from_records(offs, lens, np.full(3, E.KIND_ETH, np.uint8), "cuda:0")
    gd = torch.from_numpy(E.make_groups([0], [3]).view(np.uint8).copy()).cuda()
    st, sg, fl = eng.verify_tcp_assemble(d, batch, gd, dst, torch.from_numpy(wins.view(np.uint8).copy()).cuda())
    assert eng.last_launch()["kernel"] == "tcpasm_kernel"
    flow = fl.cpu().numpy().reshape(-1).view(E.TCPFLOW_DTYPE)[0]
    assert (int(flow["contig_len"]), int(flow["counted"]), int(flow["valid"])) == (3000, 3, 1)
    ring = dst[base:base + 3000].cpu().numpy()
    assert np.roll(ring, -2500).tobytes() == data
    assert bool((dst[:base] == R.SENTINEL).all()) and bool((dst[base + 3000:] == R.SENTINEL).all())
    del dst


def test_stream_and_empty_call(eng):
    """A non-default stream; n_groups == 0 launches nothing and writes nothing."""
    rng = np.random.default_rng(21)
    recs = [frame(1, P.rand_bytes(rng, 200)), frame(201, P.rand_bytes(rng, 200))]
    rings = Rings(10)
    rings.add(1, 400)
    _run(eng, recs, [(0, 2)], rings, stream=torch.cuda.Stream())
    d = torch.zeros(256, dtype=torch.uint8, device="cuda")
    dst = torch.full((64,), R.SENTINEL, dtype=torch.uint8, device="cuda")
    empty = torch.zeros(0, dtype=torch.uint8, device="cuda")
    eng.verify(d, E.Batch.fixed(4, 64, 64, E.KIND_IP))
    st, sg, fl = eng.verify_tcp_assemble(d, E.Batch.fixed(4, 64, 64, E.KIND_IP), empty, dst, empty,
                                         status=torch.full((4,), PRE, dtype=torch.uint8, device="cuda"))
    assert eng.last_launch()["kernel"] != "tcpasm_kernel"
    assert bool((st == PRE).all()) and bool((dst == R.SENTINEL).all()) and fl.numel() == 0
