"""GPU parity: the HIP engine (through the C ABI) against the CPU oracle, bit for bit.

Every test builds records on the host, copies them to HBM, runs smol_csum_batch_{emit,verify,data}
and compares the device bytes / status bytes / u16 outputs with oracle/csum_oracle.c on the same
input.  Coverage follows the reference's own tests (SURVEY.md §4, §8(d) edge set): the wire KATs
wrapped in IP packets, the iface IPv6 packets (odd-length ICMPv6), the fuzz-corpus Ethernet
frames, odd record offsets, every launch shape, all caps combinations, UDP/TCP computed-zero
checksums, UDP zero field on v4/v6, IPv4 options and fragments, IPv6 Hop-by-Hop (inside and
beyond the LDS header window), malformed lengths, random garbage, single-bit corruption, empty
and maximum-length records, and data() spans long enough to wrap the reference's u32 sum.
"""
import itertools

import numpy as np
import pytest

import oracle
from oracle import pyref
from tests import pktgen as P

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from smoltcp_amd import engine as E  # noqa: E402
from tests.engines import VariantEngine  # noqa: E402

CAPS_DEFAULT = (0, 0, 0, 0, 0)
V4A, V4B = bytes([192, 168, 1, 1]), bytes([192, 168, 1, 2])
SHAPES = [0, 1, 2, 3, 4, 5, 6, 7, 8]


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    e = VariantEngine(0)
    yield e
    e.close()


def _dev(buf: np.ndarray):
    return torch.from_numpy(buf.copy()).to("cuda:0")


def _run_records(eng, records, kinds, caps=CAPS_DEFAULT, gap_seed=None, shape=-1, max_blocks=0,
                 base_pad=0, variant=-1, order=None):
    """Verify and emit `records` on the device and on the oracle; assert identical results.
    `order`: a permutation of the descriptors (records stay where `pack` put them)."""
    rng = np.random.default_rng(gap_seed) if gap_seed is not None else None
    buf, offs, lens = P.pack(records, gap_rng=rng, base_pad=base_pad)
    kinds = np.broadcast_to(np.asarray(kinds, dtype=np.uint8), (len(records),)).copy()
    if order is not None:
        offs, lens, kinds = np.asarray(offs)[order], np.asarray(lens)[order], kinds[order]
    eng.set_shape(shape)
    eng.set_max_blocks(max_blocks)
    eng.set_variant(variant)
    try:
        batch = E.Batch.from_records(offs, lens, kinds, "cuda:0")
        d = _dev(buf)
        st = eng.verify(d, batch, caps=caps).cpu().numpy()
        launched_v = eng.last_launch()
        ref_st = P.oracle_verify_records(buf, offs, lens, kinds, caps)
        bad = np.nonzero(st != ref_st)[0]
        assert bad.size == 0, f"verify mismatch at {bad[:8]}: got {st[bad[:8]]} want {ref_st[bad[:8]]}"
        est = torch.zeros(len(records), dtype=torch.uint8, device="cuda:0")
        eng.emit(d, batch, caps=caps, status=est)
        launched_e = eng.last_launch()
        got = d.cpu().numpy()
        ref = buf.copy()
        ref_est = P.oracle_emit_records(ref, offs, lens, kinds, caps)
        diff = np.nonzero(got != ref)[0]
        assert diff.size == 0, f"emit bytes differ at {diff[:8]}"
        assert np.array_equal(est.cpu().numpy(), ref_est), "emit status differs"
        if variant in (56, 60, 63, 41) and len(records):  # verify ran the descriptor walk it names
            assert (launched_v["kernel"], launched_v["variant"]) == ("dwalk_kernel", 63 if variant == 41 else variant), launched_v
        if variant in (61, 62, 63, 18, 20, 41) and len(records):  # so did emit
            assert (launched_e["kernel"], launched_e["variant"]) == ("dwalk_kernel", variant), launched_e
        return st, got, offs, lens
    finally:
        eng.set_shape(-1)
        eng.set_max_blocks(0)
        eng.set_variant(-1)


# ---------------------------------------------------------------------------------------------
# Reference known-answer vectors
# ---------------------------------------------------------------------------------------------


def _wrap_kat(k):
    """Wrap an L4 KAT in the IP packet the reference's addresses imply (ipv4 KATs are whole
    packets already)."""
    b = bytes.fromhex(k["bytes"])
    proto = k["proto"]
    if proto == "ipv4":
        return b, 0
    src = bytes.fromhex(k["src"]) if k["src"] else V4A
    dst = bytes.fromhex(k["dst"]) if k["dst"] else V4B
    if proto == "icmpv6":
        return P.ipv6(src, dst, 58, b), 40
    if proto in ("udp", "tcp") and len(src) == 16:
        return P.ipv6(src, dst, 17 if proto == "udp" else 6, b), 40
    pnum = {"udp": 17, "tcp": 6, "icmpv4": 1, "igmp": 2}[proto]
    pkt = bytearray(P.ipv4(src, dst, pnum, b))
    pyref.ipv4_fill(pkt)  # a valid wrapper header, so IP_VALID is asserted too
    return bytes(pkt), 20


def test_kats_verify_and_construct(eng, golden):
    """Deconstruct: the engine's L4_VALID/IP_VALID agree with the KAT; construct: emitting over
    the pre-fill field value reproduces the reference bytes exactly."""
    recs, presets = [], []
    for k in golden["kat"]:
        pkt, l4 = _wrap_kat(k)
        recs.append(pkt)
        pre = bytearray(pkt)
        if k["pre_fill_field"] is not None:
            f = (0 if k["proto"] == "ipv4" else l4) + k["field"]
            pre[f] = k["pre_fill_field"] >> 8
            pre[f + 1] = k["pre_fill_field"] & 0xFF
        presets.append(bytes(pre))
    st, _, _, _ = _run_records(eng, recs, E.KIND_IP)
    for k, s in zip(golden["kat"], st):
        if k["proto"] == "ipv4":
            assert s & E.ST_IP_VALID, k["name"]
        else:
            assert bool(s & E.ST_L4_VALID) == k["verify"], k["name"]
            assert s & E.ST_IP_VALID and not s & E.ST_MALFORMED, k["name"]
    # construct: emit over the presets gives the KAT bytes (the IPv4 wrapper's own header is
    # filled too, so compare the L4 part; ipv4 KATs compare whole)
    _, got, offs, lens = _run_records(eng, presets, E.KIND_IP)
    for k, o, ln, pkt in zip(golden["kat"], offs, lens, recs):
        if k["pre_fill_field"] is None:
            continue
        _, l4 = _wrap_kat(k)
        rec = got[int(o):int(o) + int(ln)].tobytes()
        if k["proto"] == "ipv4":
            assert rec[:20] == pkt[:20], k["name"]
        else:
            assert rec[l4:] == bytes.fromhex(k["bytes"]), k["name"]


def test_iface_ipv6_packets(eng, golden):
    recs = [bytes.fromhex(p["bytes"]) for p in golden["iface_ipv6_packets"]]
    st, _, _, _ = _run_records(eng, recs, E.KIND_IP, gap_seed=1)
    assert all(s & E.ST_ACCEPT and s & E.ST_L4_VALID for s in st)


def test_fuzz_corpus_frames(eng, golden):
    recs = [bytes.fromhex(f["bytes"]) for f in golden["fuzz_corpus_frames"]]
    for seed in (None, 2, 3):
        _run_records(eng, recs, E.KIND_ETH, gap_seed=seed)


# ---------------------------------------------------------------------------------------------
# Synthetic batches: every profile, shape, alignment
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("profile,kind,lens", [
    (E.SYNTH_UDP4, E.KIND_IP, [28, 29, 64, 65, 1499, 1500, 1501, 4000, 9000]),
    (E.SYNTH_TCP4, E.KIND_IP, [40, 41, 64, 100, 1500, 8999, 9000]),
    (E.SYNTH_V6MIX, E.KIND_IP, [60, 61, 100, 1320, 1321, 9000]),
    (E.SYNTH_ETH_TCP4, E.KIND_ETH, [54, 55, 1514, 9014]),
])
def test_synth_profiles_fixed_stride(eng, profile, kind, lens):
    """Implicit (fixed-stride) batches, including odd strides (odd record starts), every shape."""
    for L in lens:
        for stride in (L, L + 1, L + 3):
            n = 257
            buf = torch.zeros(n * stride + 16, dtype=torch.uint8, device="cuda:0")
            batch = E.Batch.fixed(n, stride, L, kind)
            eng.synth(buf, batch, profile, seed=L * 7 + stride)
            if stride != L + 3:
                eng.emit(buf, batch)  # valid records; the L+3 stride keeps zeroed checksum fields
            eng.corrupt(buf, batch, every=5, seed=L)
            host = buf.cpu().numpy().copy()
            for shape in SHAPES:
                eng.set_shape(shape)
                st = eng.verify(buf, batch).cpu().numpy()
                ref = oracle.batch_verify(host, None, n, stride, L, kind, CAPS_DEFAULT)
                assert np.array_equal(st, ref), (profile, L, stride, shape)
                d2 = buf.clone()
                eng.emit(d2, batch)
                ref_buf = host.copy()
                oracle.batch_emit(ref_buf, None, n, stride, L, kind, CAPS_DEFAULT)
                assert np.array_equal(d2.cpu().numpy(), ref_buf), (profile, L, stride, shape)
            eng.set_shape(-1)


def test_c2_like_emit_then_verify_roundtrip(eng):
    """The bench workload at reduced n: emit -> every record ACCEPTed; 1/64 single-bit flips ->
    exactly the oracle's rejections."""
    n, L = 1 << 14, 1500
    buf = torch.empty(n * L, dtype=torch.uint8, device="cuda:0")
    batch = E.Batch.fixed(n, L, L, E.KIND_IP)
    eng.synth(buf, batch, E.SYNTH_UDP4, seed=0x5EED0001)
    eng.emit(buf, batch)
    st = eng.verify(buf, batch)
    assert bool(((st & E.ST_ACCEPT) != 0).all())
    eng.corrupt(buf, batch, every=64, seed=11)
    st = eng.verify(buf, batch).cpu().numpy()
    ref = oracle.batch_verify(buf.cpu().numpy(), None, n, L, L, E.KIND_IP, CAPS_DEFAULT)
    assert np.array_equal(st, ref)
    rejected = int(((st & E.ST_ACCEPT) == 0).sum())
    assert 0 < rejected <= n // 64 + 1


def test_packed_mixed_lengths_descriptors(eng):
    """C3-style: TCP records of random length 64..9000 packed back to back (odd offsets)."""
    rng = np.random.default_rng(0x5EED0002)
    n = 3000
    lens = rng.integers(64, 9001, n).astype(np.uint32)
    offs = np.zeros(n, dtype=np.uint64)
    offs[1:] = np.cumsum(lens[:-1].astype(np.uint64))
    total = int(offs[-1] + lens[-1]) + 16
    buf = torch.zeros(total, dtype=torch.uint8, device="cuda:0")
    batch = E.Batch.from_records(offs, lens, E.KIND_IP, "cuda:0")
    eng.synth(buf, batch, E.SYNTH_TCP4, seed=0x5EED0002)
    eng.corrupt(buf, batch, every=7, seed=3)
    host = buf.cpu().numpy().copy()
    desc = E.make_descriptors(offs, lens, E.KIND_IP)
    ref_v = oracle.batch_verify(host, desc, n)
    ref = host.copy()
    oracle.batch_emit(ref, desc, n)
    for variant in eng.avail((-1, 5, 13, 1, 7, 23, 24, 25, 26, 27, 28, 29)):
        for shape in SHAPES:
            eng.set_shape(shape)
            eng.set_variant(variant)
            try:
                st = eng.verify(buf, batch).cpu().numpy()
                d2 = buf.clone()
                eng.emit(d2, batch)
            finally:
                eng.set_shape(-1)
                eng.set_variant(-1)
            assert np.array_equal(st, ref_v), (variant, shape)
            assert np.array_equal(d2.cpu().numpy(), ref), (variant, shape)


def test_persistent_grid_small(eng):
    """Few workgroups, many records per group (exercises the register double buffer)."""
    rng = np.random.default_rng(5)
    recs = []
    for i in range(600):
        pl = P.rand_bytes(rng, int(rng.integers(0, 2000)))
        recs.append(P.ipv4(V4A, V4B, 17, P.udp(1000 + i, 53, pl)) if i % 2 else
                    P.ipv6(bytes(16), bytes([1] * 16), 6, P.tcp(1, 2, pl)))
    for shape in SHAPES:
        for mb in (1, 3):
            _run_records(eng, recs, E.KIND_IP, gap_seed=shape + 10 * mb, shape=shape, max_blocks=mb)


# ---------------------------------------------------------------------------------------------
# Policy and protocol edge cases
# ---------------------------------------------------------------------------------------------


def _mixed_records(rng, n=240):
    recs = []
    for i in range(n):
        pl = P.rand_bytes(rng, int(rng.integers(0, 300)))
        k = i % 8
        s4, d4 = P.rand_bytes(rng, 4), P.rand_bytes(rng, 4)
        s6, d6 = P.rand_bytes(rng, 16), P.rand_bytes(rng, 16)
        if k == 0:
            recs.append(P.ipv4(s4, d4, 17, P.udp(7, 9, pl)))
        elif k == 1:
            recs.append(P.ipv4(s4, d4, 6, P.tcp(7, 9, pl)))
        elif k == 2:
            recs.append(P.ipv4(s4, d4, 1, P.icmp_echo(8, pl)))
        elif k == 3:
            recs.append(P.ipv4(s4, d4, 2, bytes([0x16, 0, 0, 0]) + P.rand_bytes(rng, 4)))
        elif k == 4:
            recs.append(P.ipv6(s6, d6, 17, P.udp(7, 9, pl)))
        elif k == 5:
            recs.append(P.ipv6(s6, d6, 6, P.tcp(7, 9, pl)))
        elif k == 6:
            recs.append(P.ipv6(s6, d6, 58, P.icmp_echo(128, pl)))
        else:
            recs.append(P.ipv4(s4, d4, 6, P.tcp(7, 9, pl), ihl=int(rng.integers(5, 16)),
                               options=None))
    return recs


@pytest.mark.parametrize("variant", [56, 60, 61, 62, 63, 18, 20, 41, 94, 96, 97, 103, 104, 105, 109])
def test_dwalk_descriptor_batches(eng, variant):
    """The descriptor walks (63: the product's descriptor verify / emit, cached header windows; 60:
    non-temporal windows; experiments build: 56, and 61 / 62 = 60's / 63's emit with whole field
    segments): packed records (one wave-contiguous span per 8 records; segments reaching
    into the previous record), gapped and shuffled descriptors (one span per record),
    tiny and empty records, records of 20-60 KB, Ethernet / raw / malformed records, every caps
    gate; verify statuses and emitted bytes against the oracle."""
    eng.need(variant)
    rng = np.random.default_rng(56)
    recs = _mixed_records(rng, 400)
    for i in range(0, 400, 37):  # long records
        recs[i] = P.ipv4(V4A, V4B, 6, P.tcp(1, 2, P.rand_bytes(rng, int(rng.integers(20000, 60000)))))
    for i in range(5, 400, 41):  # tiny and empty records
        recs[i] = P.rand_bytes(rng, int(rng.integers(0, 40)))
    _run_records(eng, recs, E.KIND_IP, variant=variant)
    _run_records(eng, recs, E.KIND_IP, variant=variant, gap_seed=56)
    _run_records(eng, recs, E.KIND_IP, variant=variant, order=rng.permutation(len(recs)))
    _run_records(eng, [P.eth(r, 0x0800) for r in recs], E.KIND_ETH, variant=variant, base_pad=3)
    for caps in ((2, 3, 0, 1, 0), (1, 1, 1, 1, 1)):
        _run_records(eng, recs, E.KIND_IP, caps=caps, variant=variant, gap_seed=7)
    # C3-like: synthetic TCP segments of U[64, 9000] B packed at odd offsets
    n = 4099
    lens = rng.integers(64, 9001, n).astype(np.uint32)
    offs = np.zeros(n, dtype=np.uint64)
    offs[1:] = np.cumsum(lens[:-1].astype(np.uint64))
    total = int(offs[-1] + lens[-1]) + 16
    buf = torch.zeros(total + 1, dtype=torch.uint8, device="cuda:0")
    view = buf[1:]
    batch = E.Batch.from_records(offs, lens, E.KIND_IP, "cuda:0")
    eng.synth(view, batch, E.SYNTH_TCP4, seed=3)
    eng.emit(view, batch)
    eng.corrupt(view, batch, every=7, seed=3)
    host = view.cpu().numpy().copy()
    desc = P.oracle_desc(offs, lens, E.KIND_IP)
    eng.set_variant(variant)
    try:
        st = eng.verify(view, batch).cpu().numpy()
        eng.emit(view, batch)
        got = view.cpu().numpy()
    finally:
        eng.set_variant(-1)
    assert np.array_equal(st, oracle.batch_verify(host.copy(), desc, n))
    ref = host.copy()
    oracle.batch_emit(ref, desc, n)
    assert np.array_equal(got, ref)


def test_all_caps_combinations(eng):
    rng = np.random.default_rng(9)
    recs = _mixed_records(rng)
    # emit once with default caps so verify sees valid checksums, then flip a few
    buf, offs, lens = P.pack(recs)
    P.oracle_emit_records(buf, offs, lens, E.KIND_IP)
    valid = [buf[int(o):int(o) + int(n)].tobytes() for o, n in zip(offs, lens)]
    for i in range(0, len(valid), 5):
        b = bytearray(valid[i])
        b[-1] ^= 0x10
        valid[i] = bytes(b)
    combos = [(c,) * 5 for c in range(4)]
    all_combos = list(itertools.product(range(4), repeat=5))
    pick = np.random.default_rng(10).choice(len(all_combos), 60, replace=False)
    combos += [all_combos[i] for i in pick]
    for caps in combos:
        _run_records(eng, valid, E.KIND_IP, caps=caps, gap_seed=sum(caps))


def _force_zero(rec: bytes, l4: int, field: int, tail: int) -> bytes:
    """Adjust one 16-bit payload word so that the computed L4 checksum becomes 0."""
    buf, offs, lens = P.pack([rec])
    P.oracle_emit_records(buf, offs, lens, E.KIND_IP)
    c = int(buf[l4 + field]) << 8 | int(buf[l4 + field + 1])
    b = bytearray(rec)
    w = (b[tail] << 8 | b[tail + 1]) + c  # add c (one's complement) to a payload word
    w = (w & 0xFFFF) + (w >> 16)
    b[tail], b[tail + 1] = w >> 8, w & 0xFF
    return bytes(b)


def test_computed_zero_checksums(eng):
    """UDP: a computed 0 is sent as 0xffff (udp.rs:207); TCP: sent as 0x0000 (no mapping)."""
    rng = np.random.default_rng(4)
    recs = []
    for i in range(40):
        pl = P.rand_bytes(rng, 2 * int(rng.integers(2, 50)))
        if i % 2:
            r = P.ipv4(V4A, V4B, 17, P.udp(5, 6, pl))
            recs.append(_force_zero(r, 20, 6, 28))
        else:
            r = P.ipv6(bytes(16), bytes([2] * 16), 6, P.tcp(5, 6, pl))
            recs.append(_force_zero(r, 40, 16, 60))
    _, got, offs, lens = _run_records(eng, recs, E.KIND_IP, gap_seed=8)
    for i, (o, n) in enumerate(zip(offs, lens)):
        rec = got[int(o):int(o) + int(n)]
        if i % 2:
            assert rec[26] == 0xFF and rec[27] == 0xFF
        else:
            assert rec[56] == 0 and rec[57] == 0


def test_udp_zero_field_v4_v6(eng):
    rng = np.random.default_rng(6)
    recs = []
    for i in range(32):
        pl = P.rand_bytes(rng, int(rng.integers(0, 100)))
        recs.append(P.ipv4(V4A, V4B, 17, P.udp(5, 6, pl)) if i % 2 else
                    P.ipv6(bytes(16), bytes([3] * 16), 17, P.udp(5, 6, pl)))
    st, _, _, _ = _run_records(eng, recs, E.KIND_IP)
    # the zero field is accepted on both families (udp.rs:138-140; the IPv4 wrapper header here
    # carries checksum 0, so only the L4 bits are asserted)
    assert all(s & E.ST_L4_OK and s & E.ST_L4_VALID and not s & E.ST_MALFORMED for s in st)


def test_ipv4_fragments_and_options(eng):
    rng = np.random.default_rng(12)
    recs = []
    for i in range(60):
        pl = P.udp(1, 2, P.rand_bytes(rng, int(rng.integers(0, 64))))
        ff = [0x4000, 0x2000, 0x0001, 0x2005, 0x0000][i % 5]
        ihl = 5 + i % 11
        recs.append(P.ipv4(P.rand_bytes(rng, 4), P.rand_bytes(rng, 4), 17, pl, ihl=ihl,
                           flags_frag=ff, options=P.rand_bytes(rng, ihl * 4 - 20)))
    _run_records(eng, recs, E.KIND_IP, gap_seed=12)
    _run_records(eng, [P.eth(r) for r in recs], E.KIND_ETH, gap_seed=13)


def test_ipv6_hop_by_hop(eng):
    """One leading Hop-by-Hop header (src/iface/interface/ipv6.rs:205-211), short and long (the
    long ones put the L4 header past the 128-byte LDS window)."""
    rng = np.random.default_rng(13)
    recs = []
    for i in range(80):
        units = [0, 1, 3, 20, 60][i % 5]
        nh = [6, 17, 58, 59][i % 4]
        pl = P.rand_bytes(rng, int(rng.integers(0, 200)))
        l4 = {6: P.tcp(3, 4, pl), 17: P.udp(3, 4, pl), 58: P.icmp_echo(128, pl), 59: pl}[nh]
        recs.append(P.ipv6(P.rand_bytes(rng, 16), P.rand_bytes(rng, 16), 0,
                           P.hbh(nh, units, rng) + l4))
    _run_records(eng, recs, E.KIND_IP, gap_seed=14)
    _run_records(eng, [P.eth(r, 0x86DD) for r in recs], E.KIND_ETH, gap_seed=15)


def test_iface_ipv6_hop_by_hop_packets(eng, golden):
    """The reference's hop_by_hop_* packets (src/iface/interface/tests/ipv6.rs:151,200,232,290):
    skip -> accepted, the three discards -> MALFORMED (process_hopbyhop drops them before the L4
    gate, ipv6.rs:282-313); random gaps, every shape."""
    hbh = golden["iface_ipv6_hop_by_hop"]
    recs = [bytes.fromhex(p["bytes"]) for p in hbh] * 8
    for shape in (-1, 0, 1, 3, 5, 7, 8):
        st, _, _, _ = _run_records(eng, recs, E.KIND_IP, gap_seed=3 + shape, shape=shape)
        for p, s in zip(hbh * 8, st):
            if p["dropped"]:
                assert s & E.ST_MALFORMED and not s & E.ST_ACCEPT, (p["cite"], shape, hex(s))
            else:
                assert s & E.ST_ACCEPT and s & E.ST_L4_VALID, (p["cite"], shape, hex(s))


def test_ipv6_hop_by_hop_options(eng):
    """Random Hop-by-Hop options (Pad1, PadN, RouterAlert of right and wrong length, unknown types of
    every failure action, Rpl, truncated TLVs, more than 4 options) against the oracle, on IP and
    Ethernet records, fixed-stride and descriptor batches; options behind long PadN fillers put the
    tested options past the LDS window."""
    rng = np.random.default_rng(21)
    recs = []
    for i in range(400):
        opts = P.random_hbh_options(rng)
        if i % 5 == 4:  # two long PadN options first: the tested options sit past the window
            opts = bytes([1, 250]) + bytes(250) + bytes([1, 120]) + bytes(120) + opts
        nh = [6, 17, 58][i % 3]
        pl = P.rand_bytes(rng, int(rng.integers(0, 120)))
        l4 = {6: P.tcp(3, 4, pl), 17: P.udp(3, 4, pl), 58: P.icmp_echo(128, pl)}[nh]
        recs.append(P.ipv6(P.rand_bytes(rng, 16), P.rand_bytes(rng, 16), 0, P.hbh_opts(nh, opts) + l4))
    # emit first (valid checksums), so that verify's status says whether the options dropped it
    buf, offs, lens = P.pack(recs)
    P.oracle_emit_records(buf, offs, lens, np.full(len(recs), E.KIND_IP, np.uint8), CAPS_DEFAULT)
    recs = [buf[int(o):int(o) + int(n)].tobytes() for o, n in zip(offs, lens)]
    st, _, _, _ = _run_records(eng, recs, E.KIND_IP, gap_seed=22)
    dropped = sum(bool(s & E.ST_MALFORMED) for s in st)
    assert 0.2 * len(recs) < dropped < 0.9 * len(recs), dropped
    _run_records(eng, [P.eth(r, 0x86DD) for r in recs], E.KIND_ETH, gap_seed=23, shape=1)
    # fixed stride: the records padded to one length
    L = max(len(r) for r in recs)
    fixed = [r + bytes(L - len(r)) for r in recs]
    host = np.frombuffer(b"".join(fixed) + bytes(16), dtype=np.uint8).copy()
    d = _dev(host)
    batch = E.Batch.fixed(len(fixed), L, L, E.KIND_IP)
    st = eng.verify(d, batch).cpu().numpy()
    ref = oracle.batch_verify(host, None, len(fixed), L, L, E.KIND_IP, CAPS_DEFAULT)
    assert np.array_equal(st, ref)


def test_malformed_and_garbage(eng):
    """Length-field lies, truncation, wrong versions, random bytes: statuses match, and emit
    writes exactly where the oracle writes."""
    rng = np.random.default_rng(14)
    recs = []
    for i in range(400):
        pl = P.rand_bytes(rng, int(rng.integers(0, 120)))
        base = [P.ipv4(V4A, V4B, 17, P.udp(1, 2, pl)), P.ipv4(V4A, V4B, 6, P.tcp(1, 2, pl)),
                P.ipv6(bytes(16), bytes(16), 58, P.icmp_echo(128, pl)),
                P.ipv6(bytes(16), bytes(16), 17, P.udp(1, 2, pl))][i % 4]
        b = bytearray(base)
        mode = i % 10
        if mode == 0:
            b = b[: int(rng.integers(0, len(b) + 1))]  # truncated
        elif mode == 1:
            j = int(rng.integers(0, min(len(b), 64)))
            b[j] = int(rng.integers(0, 256))  # header byte garbage
        elif mode == 2:
            b = bytearray(P.rand_bytes(rng, int(rng.integers(0, 200))))
        elif mode == 3:
            b += P.rand_bytes(rng, int(rng.integers(1, 40)))  # trailing padding
        recs.append(bytes(b))
    for kind in (E.KIND_IP, E.KIND_ETH, E.KIND_RAW):
        _run_records(eng, recs, kind, gap_seed=kind)


# ---------------------------------------------------------------------------------------------
# data(): raw spans
# ---------------------------------------------------------------------------------------------


def test_data_raw_spans(eng):
    rng = np.random.default_rng(15)
    lens = list(range(0, 80)) + [1499, 1500, 1501, 4095, 4096, 9000, 65535, 65536, 131074,
                                 131075, 200003]
    recs = [P.rand_bytes(rng, n) for n in lens]
    recs += [bytes(n) for n in (0, 1, 7, 64, 1500)] + [b"\xff" * n for n in (1, 2, 63, 1500, 131076, 262150)]
    for shape in SHAPES:
        buf, offs, lens_a = P.pack(recs, gap_rng=np.random.default_rng(shape))
        batch = E.Batch.from_records(offs, lens_a, E.KIND_RAW, "cuda:0")
        eng.set_shape(shape)
        out = eng.data(_dev(buf), batch).cpu().numpy().view(np.uint16)
        ref = P.oracle_data_records(buf, offs, lens_a)
        assert np.array_equal(out, ref), (shape, np.nonzero(out != ref)[0][:8])
    eng.set_shape(-1)


def test_data_fixed_stride_large(eng):
    """1 MiB spans of 0xff wrap the reference's u32 accumulator many times over."""
    for fill in (0xFF, None):
        n, L = 6, 1 << 20
        if fill is None:
            host = np.random.default_rng(16).integers(0, 256, n * L + 16, dtype=np.uint8)
        else:
            host = np.full(n * L + 16, fill, dtype=np.uint8)
        for stride in (L, L + 1):
            nn = (host.size - 16 - L) // stride + 1
            out = eng.data(_dev(host), E.Batch.fixed(nn, stride, L, E.KIND_RAW)).cpu().numpy().view(np.uint16)
            ref = oracle.batch_data(host, None, nn, stride, L)
            assert np.array_equal(out, ref), stride


def test_empty_batch_and_errors(eng):
    buf = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
    eng.verify(buf, E.Batch.fixed(0, 0, 0))  # n == 0 is a no-op
    with pytest.raises(Exception):
        eng.verify(buf, E.Batch.fixed(1, 16, 16), caps=(9, 0, 0, 0, 0))


def test_grid_cap_huge_batch(eng):
    """2^27 records with 64-lane groups want more than 2^32 work-items: the launcher caps the grid
    and the kernels' grid-stride loop still covers every record (C5 sizes)."""
    rec = np.frombuffer(P.ipv4(V4A, V4B, 17, P.udp(1, 2, bytes(range(36)))), np.uint8)
    buf = rec.copy()
    oracle.batch_emit(buf, None, 1, 64, 64, 1)
    d = torch.from_numpy(np.concatenate([buf, np.zeros(16, np.uint8)])).cuda()
    n = 1 << 27
    eng.set_shape(6)
    try:
        st = eng.verify(d, E.Batch.fixed(n, 0, len(rec), E.KIND_IP))
    finally:
        eng.set_shape(-1)
    ref = oracle.batch_verify(buf.copy(), None, 1, 64, len(rec), 1)[0]
    assert int((st == int(ref)).sum()) == n and (ref & E.ST_ACCEPT)


def _emit_case(eng, host, off, n, stride, L, kind, caps, variant, shape=-1, blocks=0):
    """Emit a fixed-stride batch that starts `off` bytes into `host` (a device copy of it) and
    compare the WHOLE buffer with the oracle: bytes outside the records (before the batch, gaps,
    neighbours' lines) must not change."""
    full = torch.from_numpy(host.copy()).cuda()
    d = full[off:]
    batch = E.Batch.fixed(n, stride, L, kind)
    st = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    eng.set_variant(variant)
    eng.set_shape(shape)
    eng.set_max_blocks(blocks)
    try:
        eng.emit(d, batch, caps=caps, status=st)
        launched = eng.last_launch()
        got = full.cpu().numpy()
    finally:
        eng.set_variant(-1)
        eng.set_shape(-1)
        eng.set_max_blocks(0)
    if variant >= 0:
        assert _kv(launched) == _expected_launch(variant, "emit", False), (variant, launched)
    ref = host.copy()
    sub = ref[off:].copy()
    ref_st = oracle.batch_emit(sub, None, n, stride, L, kind, caps)
    ref[off:] = sub
    diff = np.nonzero(got != ref)[0]
    assert diff.size == 0, (stride, L, off, variant, shape, blocks, caps, diff[:8])
    assert np.array_equal(st.cpu().numpy(), ref_st), (stride, L, off, variant)


@pytest.mark.parametrize("profile,kind", [(E.SYNTH_UDP4, E.KIND_IP), (E.SYNTH_TCP4, E.KIND_IP),
                                          (E.SYNTH_V6MIX, E.KIND_IP), (E.SYNTH_ETH_TCP4, E.KIND_ETH)])
def test_emit_variants_match_oracle(eng, profile, kind):
    """Fixed-stride emit in every kernel variant (line grid with shared boundary lines — the
    default — cached field lines, 16-byte grid, cached / non-temporal loads) against the oracle
    over the whole buffer: short, odd and line-sized strides, odd batch starts, gaps (stride > len),
    every shape, persistent grids, caps that write zeros."""
    rng = np.random.default_rng(profile)
    for stride, L in [(64, 64), (97, 97), (200, 200), (255, 255), (256, 256), (257, 257), (300, 256),
                      (1500, 1500), (1501, 1501), (1519, 1500), (4000, 4000)]:
        n = 1031
        for off in (0, 37):
            host = rng.integers(0, 256, off + n * stride + 128, dtype=np.uint8)
            tmp = torch.from_numpy(host[off:].copy()).cuda()
            eng.synth(tmp, E.Batch.fixed(n, stride, L, kind), profile, seed=stride * 13 + profile + off)
            host[off:] = tmp.cpu().numpy()
            for variant, shape, blocks, caps in [
                    (-1, -1, 0, (0, 0, 0, 0, 0)), (5, 0, 3, (0, 0, 0, 0, 0)),
                    (6, 1, 0, (2, 3, 0, 1, 0)), (5, 7, 0, (0, 0, 0, 0, 0)),
                    (5, 8, 5, (3, 2, 2, 3, 3)), (9, 5, 0, (0, 0, 0, 0, 0)),
                    (10, 7, 0, (0, 0, 0, 0, 0)), (1, 3, 0, (0, 0, 0, 0, 0)), (0, 0, 0, (0, 0, 0, 0, 0)),
                    (19, -1, 0, (0, 0, 0, 0, 0)), (19, 7, 3, (3, 2, 2, 3, 3)), (19, 0, 5, (2, 3, 0, 1, 0)),
                    (23, -1, 0, (0, 0, 0, 0, 0)), (23, 7, 3, (3, 2, 2, 3, 3)), (23, 0, 5, (2, 3, 0, 1, 0)),
                    (24, -1, 0, (0, 0, 0, 0, 0)), (25, 7, 0, (0, 0, 0, 0, 0)), (26, -1, 0, (0, 0, 0, 0, 0)),
                    (26, 1, 3, (2, 3, 0, 1, 0)), (27, 8, 0, (0, 0, 0, 0, 0)), (28, 8, 5, (0, 0, 0, 0, 0)),
                    (29, -1, 0, (0, 0, 0, 0, 0)), (29, 7, 3, (3, 2, 2, 3, 3)),
                    (37, -1, 0, (0, 0, 0, 0, 0)), (37, 7, 3, (3, 2, 2, 3, 3)), (37, 0, 0, (2, 3, 0, 1, 0)),
                    (38, -1, 0, (0, 0, 0, 0, 0)), (38, 0, 5, (0, 0, 0, 0, 0)),
                    (39, -1, 0, (0, 0, 0, 0, 0)), (39, 7, 3, (3, 2, 2, 3, 3)), (39, 0, 5, (2, 3, 0, 1, 0)),
                    (40, -1, 0, (0, 0, 0, 0, 0)), (40, 7, 3, (3, 2, 2, 3, 3))]:
                if not eng.has(variant):
                    continue
                _emit_case(eng, host, off, n, stride, L, kind, caps, variant, shape, blocks)


def test_emit_neighbour_fields(eng):
    """Records whose L4 checksum field sits in their last 64 bytes (IPv6 Hop-by-Hop pushes it
    there, into the boundary line the next record's group loads) alternate with IPv4 / IPv6
    records whose field lines start in the previous record's last line."""
    rng = np.random.default_rng(77)
    a6, b6 = bytes(range(16)), bytes(range(16, 32))
    for stride in (256, 257, 300, 301, 320):
        recs = []
        for i in range(515):
            k = i % 3
            if k == 0:  # UDP field near the record end
                units = (stride - 40 - 8 - 10) // 8 - 1
                h = P.hbh(17, units, rng)
                room = stride - 40 - len(h) - 8
                body = P.ipv6(a6, b6, 0, h + P.udp(5, 6, P.rand_bytes(rng, int(rng.integers(0, room + 1)))))
            elif k == 1:
                body = P.ipv4(V4A, V4B, 17, P.udp(1, 2, P.rand_bytes(rng, int(rng.integers(0, stride - 28)))))
            else:
                body = P.ipv6(a6, b6, 6, P.tcp(7, 8, P.rand_bytes(rng, int(rng.integers(0, stride - 60)))))
            recs.append(body + P.rand_bytes(rng, stride - len(body)))
        n = len(recs)
        for off in (0, 5, 40, 63):
            host = np.concatenate([rng.integers(0, 256, off, dtype=np.uint8),
                                   np.frombuffer(b"".join(recs), np.uint8), np.zeros(128, np.uint8)])
            for variant in eng.avail((-1, 5, 6, 1, 0, 9, 19, 23, 24, 25, 26, 27, 28, 29)):
                _emit_case(eng, host, off, n, stride, stride, E.KIND_IP, CAPS_DEFAULT, variant)
            # whole field segments with several records per group (neighbours out of step)
            for blocks in (1, 3, 5):
                for variant in eng.avail((19, 23, 26, 28, 29, 39)):
                    _emit_case(eng, host, off, n, stride, stride, E.KIND_IP, CAPS_DEFAULT, variant, -1, blocks)


def test_emit_large_batch(eng):
    """More than 2^20 records at short strides (256 / 257 B: many records per group's line
    window neighbourhood), the whole buffer against the oracle."""
    n, L = (1 << 20) + 37, 256
    for stride, off in ((256, 0), (257, 11)):
        host = np.zeros(off + n * stride + 128, dtype=np.uint8)
        tmp = torch.zeros(n * stride + 128, dtype=torch.uint8, device="cuda:0")
        eng.synth(tmp, E.Batch.fixed(n, stride, L, E.KIND_IP), E.SYNTH_UDP4, seed=stride)
        host[off:] = tmp.cpu().numpy()
        del tmp
        _emit_case(eng, host, off, n, stride, L, E.KIND_IP, CAPS_DEFAULT, -1)


def _kv(launched):
    return (launched["kernel"], launched["variant"])


def _expected_launch(variant, op, has_desc):
    """The kernel instantiation a forced `variant` must run (csum_walk.h launch_walk, csum_api.cpp
    run_one): (kernel, VAR template argument)."""
    if variant in (3, 4, 7):
        return ("csum_tile_kernel", {3: 0, 4: 1, 7: 2}[variant])
    emit_fixed = op == "emit" and not has_desc
    if variant in (9, 10, 12, 14, 29, 37, 38, 39):
        return ("csum_kernel", variant if emit_fixed else 5)
    if variant == 62:  # the descriptor walk over fixed strides (experiments build; verify: 63)
        return ("dwalk_kernel", 62 if op == "emit" else 63)
    if 23 <= variant <= 28:
        if op == "emit":
            return ("csum_kernel", variant)
        return ("csum_kernel", 13 if variant >= 26 else 5)
    return ("csum_kernel", variant)


FIXED_STRIDE_VARIANTS = [0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 12, 13, 14, 19, 23, 24, 25, 26, 27, 28, 29, 37, 38, 39, 62]


@pytest.mark.parametrize("variant", FIXED_STRIDE_VARIANTS)
def test_variants_fixed_stride(eng, variant):
    """The non-default kernel variants (walk: nt + prefetch, nt only; tile: nt, plain loads) against
    the oracle on fixed-stride batches: strides equal to the record length (neighbours share
    lines), odd strides, gaps, every shape, natural and persistent grids."""
    eng.need(variant)
    for profile, kind, L in [(E.SYNTH_UDP4, E.KIND_IP, 1500), (E.SYNTH_V6MIX, E.KIND_IP, 1320),
                             (E.SYNTH_TCP4, E.KIND_IP, 97), (E.SYNTH_ETH_TCP4, E.KIND_ETH, 1514),
                             (E.SYNTH_UDP4, E.KIND_IP, 128), (E.SYNTH_TCP4, E.KIND_IP, 4000)]:
        for stride in (L, L + 1, L + 16):
            n = 1029
            buf = torch.zeros(n * stride + 64, dtype=torch.uint8, device="cuda:0")
            batch = E.Batch.fixed(n, stride, L, kind)
            eng.synth(buf, batch, profile, seed=L + stride + variant)
            eng.emit(buf, batch)
            eng.corrupt(buf, batch, every=7, seed=L)
            host = buf.cpu().numpy().copy()
            ref_v = oracle.batch_verify(host.copy(), None, n, stride, L, kind, CAPS_DEFAULT)
            ref_e = host.copy()
            ref_es = oracle.batch_emit(ref_e, None, n, stride, L, kind, CAPS_DEFAULT)
            for shape in SHAPES:
                for blocks in (0, 7):
                    eng.set_variant(variant)
                    eng.set_shape(shape)
                    eng.set_max_blocks(blocks)
                    try:
                        st = eng.verify(buf, batch).cpu().numpy()
                        launched_v = eng.last_launch()
                        d2 = buf.clone()
                        est = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
                        eng.emit(d2, batch, status=est)
                        launched_e = eng.last_launch()
                        got = d2.cpu().numpy()
                    finally:
                        eng.set_variant(-1)
                        eng.set_shape(-1)
                        eng.set_max_blocks(0)
                    assert _kv(launched_v) == _expected_launch(variant, "verify", False), launched_v
                    assert _kv(launched_e) == _expected_launch(variant, "emit", False), launched_e
                    assert np.array_equal(st, ref_v), (variant, L, stride, shape, blocks)
                    assert np.array_equal(got, ref_e), (variant, L, stride, shape, blocks)
                    assert np.array_equal(est.cpu().numpy(), ref_es)


WIDE_KERNELS = {
    # variant: (kernel name, the largest record length it serves)
    42: ("csum_tile_kernel", 1520),
    44: ("xwalk_kernel", 16257),
    15: ("xwalk_kernel", 16257),
    45: ("xwalk_kernel", 16257),
    46: ("xwalk_kernel", 16257),
    47: ("xwalk_kernel", 16257),
    57: ("xwalk_kernel", 16257),
    89: ("xwalk_kernel", 16257),  # the verify table's 'h': lanes 0-3 of each record's first load cached (emit: 57's form)
    101: ("xwalk_kernel", 16257),  # 57 with write-through segment stores (late round 6)
    107: ("xwalk_kernel", 16257),  # 89 in 512-thread workgroups (verify; emit 101)
    113: ("xwalk_kernel", 16257),  # two tiles per workgroup (89 / 101)
    100: ("xwalk_kernel", 16257),
    80: ("xwalk_kernel", 16257),  # staged emit: field entries, then the segment pass (round 6)
    81: ("xwalk_kernel", 16257),
    48: ("xwalk_kernel", 16257),
    59: ("xwalk_kernel", 16257),
}


@pytest.mark.parametrize("variant", sorted(WIDE_KERNELS))
def test_wide_record_kernels(eng, variant):
    """The experiment kernels for packed fixed-stride records of 1024 bytes and more (variant 42,
    the stripe kernel: a wavefront streams 8 records as wave-contiguous 1-KiB pieces; variant 44, the
    transposed walk: the same loads with the walk kernel's per-record parse and finish, 8 / 4 / 2 / 1
    records per wavefront up to 1921 / 3969 / 8065 / 16257 B; 47: 44 with whole field segments) against the
    oracle: every profile, odd record lengths (odd starts), batch sizes that leave a partial last
    wavefront, 1/7 corrupted, caps variants; the whole buffer is compared after emit.  Batches they
    do not serve (gapped strides, other lengths, descriptor batches) fall back to the walk kernel."""
    eng.need(variant)
    kname, lmax = WIDE_KERNELS[variant]
    lens = [(E.SYNTH_UDP4, E.KIND_IP, 1500), (E.SYNTH_UDP4, E.KIND_IP, 1024),
            (E.SYNTH_V6MIX, E.KIND_IP, 1320), (E.SYNTH_TCP4, E.KIND_IP, 1499),
            (E.SYNTH_ETH_TCP4, E.KIND_ETH, 1514), (E.SYNTH_TCP4, E.KIND_IP, 1025),
            (E.SYNTH_V6MIX, E.KIND_IP, 1519), (E.SYNTH_UDP4, E.KIND_IP, 1520)]
    if lmax > 1520:  # every records-per-wavefront form, at both ends of its range
        lens += [(E.SYNTH_V6MIX, E.KIND_IP, 1777), (E.SYNTH_TCP4, E.KIND_IP, 1921), (E.SYNTH_UDP4, E.KIND_IP, 1922),
                 (E.SYNTH_V6MIX, E.KIND_IP, 3001), (E.SYNTH_TCP4, E.KIND_IP, 3969), (E.SYNTH_ETH_TCP4, E.KIND_ETH, 3970),
                 (E.SYNTH_UDP4, E.KIND_IP, 8065), (E.SYNTH_V6MIX, E.KIND_IP, 8066), (E.SYNTH_TCP4, E.KIND_IP, lmax),
                 (E.SYNTH_UDP4, E.KIND_RAW, 2000)]
    for profile, kind, L in lens:
        for n, off in ((1, 0), (7, 3), (8, 0), (9, 64), (257, 1), (4099 if L < 4000 else 1029, 17)):
            host = np.zeros(off + n * L + 128, dtype=np.uint8)
            tmp = torch.zeros(n * L + 64, dtype=torch.uint8, device="cuda:0")
            batch = E.Batch.fixed(n, L, L, kind)
            eng.synth(tmp, batch, profile, seed=L * 3 + n)
            eng.emit(tmp, batch)
            eng.corrupt(tmp, batch, every=7, seed=n)
            host[off:off + tmp.numel()] = tmp.cpu().numpy()
            for caps in (CAPS_DEFAULT, (2, 3, 0, 1, 0)):
                _wide_case(eng, variant, kname, host, off, n, L, kind, caps)
    if kname == "xwalk_kernel":  # gapped strides, random bytes in the gaps
        rng = np.random.default_rng(variant)
        for profile, L in ((E.SYNTH_UDP4, 1024), (E.SYNTH_UDP4, 1500), (E.SYNTH_V6MIX, 2500), (E.SYNTH_TCP4, 5000),
                           (E.SYNTH_V6MIX, 9000)):
            for gap in (1, 63, 200):
                stride = L + gap
                for n, off in ((9, 1), (1029, 0)):
                    tmp = torch.zeros(n * L + 64, dtype=torch.uint8, device="cuda:0")
                    pb = E.Batch.fixed(n, L, L, E.KIND_IP)
                    eng.synth(tmp, pb, profile, seed=L + gap + n)
                    eng.emit(tmp, pb)
                    eng.corrupt(tmp, pb, every=7, seed=n)
                    recs = tmp.cpu().numpy()[: n * L].reshape(n, L)
                    host = rng.integers(0, 256, off + n * stride + 128, dtype=np.uint8)
                    for i in range(n):
                        host[off + i * stride: off + i * stride + L] = recs[i]
                    _wide_case(eng, variant, kname, host, off, n, L, E.KIND_IP, CAPS_DEFAULT, stride)
    # not served: a length outside the kernel's range -> the walk kernel
    stripe_gap = ((1500, 1501),) if kname != "xwalk_kernel" else ()
    for L, stride in stripe_gap + ((1000, 1000), (lmax + 1, lmax + 1)):
        n = 100
        buf = torch.zeros(n * stride + 64, dtype=torch.uint8, device="cuda:0")
        batch = E.Batch.fixed(n, stride, L, E.KIND_IP)
        eng.synth(buf, batch, E.SYNTH_UDP4, seed=L)
        host = buf.cpu().numpy().copy()
        eng.set_variant(variant)
        try:
            st = eng.verify(buf, batch).cpu().numpy()
            assert eng.last_launch()["kernel"] == "csum_kernel"
        finally:
            eng.set_variant(-1)
        assert np.array_equal(st, oracle.batch_verify(host, None, n, stride, L, E.KIND_IP, CAPS_DEFAULT))


@pytest.mark.parametrize("variant", [80, 81])
def test_staged_emit_chunks(eng, variant):
    """The staged emit over more records than one staging chunk (kStageChunk = 2^21: several staging
    launch + segment pass pairs, the context's entry buffer grown from a small first batch) writes the
    same bytes as the transposed walk's in-place emit (variant 57, oracle-checked by the tests above), and
    the oracle agrees on runs of records at the chunk seams."""
    eng.need(variant)
    L, n = 1024, (1 << 21) * 2 + 37
    b = E.Batch.fixed(n, L, L, E.KIND_IP)
    buf = torch.zeros(n * L + 64, dtype=torch.uint8, device="cuda:0")
    eng.synth(buf, b, E.SYNTH_UDP4, seed=99)
    small = E.Batch.fixed(100, L, L, E.KIND_IP)
    ref = buf.clone()
    eng.set_variant(57)
    try:
        eng.emit(ref, b)
    finally:
        eng.set_variant(-1)
    got = buf.clone()
    eng.set_variant(variant)
    try:
        eng.emit(got[: 100 * L + 64].clone(), small)  # the entry buffer first sized for 100 records
        eng.emit(got, b)
        assert (eng.last_launch()["kernel"], eng.last_launch()["variant"]) == ("xwalk_kernel", variant)
    finally:
        eng.set_variant(-1)
    torch.cuda.synchronize()
    assert torch.equal(got, ref)
    host = buf.cpu().numpy()
    for lo in (0, (1 << 21) - 40, (1 << 22) - 40, n - 60):
        hi = min(n, lo + 80)
        want = host[lo * L: hi * L].copy()
        oracle.batch_emit(want, None, hi - lo, L, L, E.KIND_IP, CAPS_DEFAULT)
        assert np.array_equal(got[lo * L: hi * L].cpu().numpy(), want), lo


def test_staged_descriptor_emit_chunks(eng):
    """The staged descriptor-batch emit (variant 94: field entries, then the segment pass) over more
    descriptors than one staging chunk (2^21), short packed records at odd offsets and shuffled ones,
    writes the same bytes as the in-place descriptor emit (variant 41, oracle-checked above), and the
    oracle agrees on records at the chunk seams."""
    eng.need(94)
    rng = np.random.default_rng(94)
    n = (1 << 21) + 4099
    lens = rng.integers(64, 200, n).astype(np.uint32)
    offs = np.zeros(n, dtype=np.uint64)
    offs[1:] = np.cumsum(lens[:-1].astype(np.uint64))
    total = int(offs[-1] + lens[-1]) + 16
    for order in (None, rng.permutation(n)):
        o, l = (offs, lens) if order is None else (offs[order], lens[order])
        batch = E.Batch.from_records(o, l, E.KIND_IP, "cuda:0")
        base = torch.zeros(total + 1, dtype=torch.uint8, device="cuda:0")
        view = base[1:]
        eng.synth(view, batch, E.SYNTH_TCP4, seed=9)
        ref = base.clone()
        eng.set_variant(41)
        try:
            eng.emit(ref[1:], batch)
        finally:
            eng.set_variant(-1)
        eng.set_variant(94)
        try:
            eng.emit(view, batch)
            assert (eng.last_launch()["kernel"], eng.last_launch()["variant"]) == ("dwalk_kernel", 94)
        finally:
            eng.set_variant(-1)
        torch.cuda.synchronize()
        assert torch.equal(base, ref)
    host = synth_host = None
    base = torch.zeros(total + 1, dtype=torch.uint8, device="cuda:0")
    batch = E.Batch.from_records(offs, lens, E.KIND_IP, "cuda:0")
    eng.synth(base[1:], batch, E.SYNTH_TCP4, seed=10)
    synth_host = base[1:].cpu().numpy().copy()
    eng.set_variant(94)
    try:
        eng.emit(base[1:], batch)
    finally:
        eng.set_variant(-1)
    host = base[1:].cpu().numpy()
    for lo in (0, (1 << 21) - 50, n - 60):
        hi = min(n, lo + 100)
        a, b = int(offs[lo]), int(offs[hi - 1] + lens[hi - 1])
        want = synth_host[a:b].copy()
        d = P.oracle_desc(offs[lo:hi] - np.uint64(a), lens[lo:hi], E.KIND_IP)
        oracle.batch_emit(want, d, hi - lo, 0, 0, E.KIND_IP, CAPS_DEFAULT)
        assert np.array_equal(host[a:b], want), lo


def _wide_case(eng, variant, kname, host, off, n, L, kind, caps, stride=None):
    stride = stride or L
    batch = E.Batch.fixed(n, stride, L, kind)
    d = torch.from_numpy(host.copy()).cuda()
    view = d[off:]
    eng.set_variant(variant)
    try:
        st = eng.verify(view, batch, caps=caps).cpu().numpy()
        lv = eng.last_launch()
        eng.emit(view, batch, caps=caps)
        le = eng.last_launch()
    finally:
        eng.set_variant(-1)
    assert (lv["kernel"], lv["variant"]) == (kname, variant), lv
    assert (le["kernel"], le["variant"]) == (kname, variant), le
    ref_v = oracle.batch_verify(host[off:].copy(), None, n, stride, L, kind, caps)
    assert np.array_equal(st, ref_v), (L, stride, n, off, caps, np.nonzero(st != ref_v)[0][:8])
    ref_e = host.copy()
    oracle.batch_emit(ref_e[off:], None, n, stride, L, kind, caps)
    got = d.cpu().numpy()
    assert np.array_equal(got, ref_e), (L, stride, n, off, caps, np.nonzero(got != ref_e)[0][:8])


@pytest.mark.parametrize("variant", sorted(WIDE_KERNELS))
def test_wide_record_kernels_edge_records(eng, variant):
    """The same kernels on records whose checksummed span ends before the record's end (IP total
    length / UDP length below the slot, random trailing bytes), truncated and garbage headers, IPv6
    Hop-by-Hop options past the LDS window, zero-length payloads: slots of 1024 .. the largest
    length, packed, verify after emit and after corruption, against the oracle."""
    eng.need(variant)
    kname, lmax = WIDE_KERNELS[variant]
    rng = np.random.default_rng(43 + variant)
    for L in sorted({1024, 1100, 1337, 1500, min(lmax, 1921), min(lmax, 2600), min(lmax, 5000), lmax}):
        recs = []
        for i in range(300):
            pl = P.rand_bytes(rng, int(rng.integers(0, L - 120)))
            m = i % 8
            if m == 0:
                r = P.ipv4(V4A, V4B, 17, P.udp(1, 2, pl))
            elif m == 1:
                r = P.ipv4(V4A, V4B, 6, P.tcp(1, 2, pl))
            elif m == 2:
                r = P.ipv6(P.rand_bytes(rng, 16), P.rand_bytes(rng, 16), 58, P.icmp_echo(128, pl))
            elif m == 3:
                opts = bytes([1, 250]) + bytes(250) + P.random_hbh_options(rng)
                r = P.ipv6(P.rand_bytes(rng, 16), P.rand_bytes(rng, 16), 0, P.hbh_opts(17, opts) + P.udp(3, 4, pl[:400]))
            elif m == 4:
                u = bytearray(P.udp(1, 2, pl))
                ul = int(rng.integers(8, len(u) + 1))  # UDP length below the IP payload
                u[4:6] = ul.to_bytes(2, "big")
                r = P.ipv4(V4A, V4B, 17, bytes(u))
            elif m == 5:
                r = P.ipv4(V4A, V4B, 17, P.udp(1, 2, b""))
            elif m == 6:
                r = P.rand_bytes(rng, int(rng.integers(0, L + 1)))
            else:
                r = P.ipv6(bytes(16), bytes(16), 6, P.tcp(1, 2, pl))[: int(rng.integers(0, 80))]
            r = r[:L]
            recs.append(r + P.rand_bytes(rng, L - len(r)))
        host = np.frombuffer(b"".join(recs) + bytes(128), dtype=np.uint8).copy()
        n = len(recs)
        P.oracle_emit_records(host, np.arange(n) * L, np.full(n, L), np.full(n, E.KIND_IP, np.uint8), CAPS_DEFAULT)
        for k in range(0, n, 5):  # every fifth record: one byte inside its first 1 KiB flipped
            host[k * L + int(rng.integers(0, 1024))] ^= 0x5A
        for off in (0, 1):
            h = np.concatenate([np.zeros(off, np.uint8), host])
            _wide_case(eng, variant, kname, h, off, n, L, E.KIND_IP, CAPS_DEFAULT)


def test_pretty_print_annotations(eng, golden):
    """The pretty-print path's checksum annotations (checksum::format_checksum, src/wire/ip.rs:
    871-886) from the DEVICE verify status: the module example of src/wire/pretty_print.rs reads
    "(checksum incorrect)" on its IPv4 line, the corpus frames with TX-offload partial checksums
    "(partial checksum correct)" on their TCP line."""
    from smoltcp_amd import checksum

    ex = golden["pretty_print"][0]
    recs = [bytes.fromhex(ex["bytes"])] + [bytes.fromhex(f["bytes"]) for f in golden["fuzz_corpus_frames"]]
    st, _, _, _ = _run_records(eng, recs, E.KIND_ETH, gap_seed=5)
    assert checksum.ipv4_annotation(int(st[0])) == ex["ipv4_annotation"] == " (checksum incorrect)"
    partial = {"tcpv4_data.bin", "tcpv4_fin.bin", "tcpv4_syn.bin"}
    for f, s in zip(golden["fuzz_corpus_frames"], st[1:]):
        want = " (partial checksum correct)" if f["name"] in partial else ""
        assert checksum.l4_annotation(int(s)) == want, f["name"]


@pytest.mark.parametrize("xcd", [0, 1, 2, 7, 64])
def test_xcd_remap(eng, xcd):
    """The XCD-contiguous block order (smol_csum_tool_set_xcd_remap) is a bijection on the grid's
    blocks: emit / verify over fixed-stride and descriptor batches whose block counts are and are not
    multiples of 8 match the oracle, natural and capped grids."""
    rng = np.random.default_rng(91)
    eng.set_xcd_remap(xcd)
    try:
        for n in (1, 31, 32 * 8, 32 * 8 + 1, 32 * 13 + 5, 4099):
            L = 1500
            buf = torch.zeros(n * L + 64, dtype=torch.uint8, device="cuda:0")
            batch = E.Batch.fixed(n, L, L, E.KIND_IP)
            eng.synth(buf, batch, E.SYNTH_UDP4, seed=n)
            eng.corrupt(buf, batch, every=5, seed=n)
            host = buf.cpu().numpy().copy()
            ref_v = oracle.batch_verify(host.copy(), None, n, L, L, E.KIND_IP, CAPS_DEFAULT)
            ref_e = host.copy()
            oracle.batch_emit(ref_e, None, n, L, L, E.KIND_IP, CAPS_DEFAULT)
            for blocks in (0, 3, 9):
                eng.set_max_blocks(blocks)
                try:
                    st = eng.verify(buf, batch).cpu().numpy()
                    d2 = buf.clone()
                    eng.emit(d2, batch)
                finally:
                    eng.set_max_blocks(0)
                assert np.array_equal(st, ref_v), (xcd, n, blocks)
                assert np.array_equal(d2.cpu().numpy(), ref_e), (xcd, n, blocks)
        recs = [P.ipv4(V4A, V4B, 6, P.tcp(1, 2, P.rand_bytes(rng, int(rng.integers(0, 3000))))) for _ in range(1029)]
        _run_records(eng, recs, E.KIND_IP, gap_seed=4)  # verify: walk kernel, emit: tile kernel
        # copy-emit (copy_kernel) under the same order
        n, L = 2053, 1500
        buf = torch.empty(n * L, dtype=torch.uint8, device="cuda:0")
        batch = E.Batch.fixed(n, L, kind=E.KIND_IP)
        eng.synth(buf, batch, E.SYNTH_UDP4, seed=xcd)
        host = buf.cpu().numpy().copy()
        src = rng.integers(0, 256, n * 1472 + 16, dtype=np.uint8)
        copies = E.make_copies(np.arange(n, dtype=np.uint64) * 1472, 28, 1472)
        eng.copy_emit(buf, batch, torch.from_numpy(src).cuda(), torch.from_numpy(copies.view(np.uint8).copy()).cuda())
        ref = host.copy()
        oracle.batch_copy_emit(ref, None, n, src, copies, L, L, E.KIND_IP)
        assert np.array_equal(buf.cpu().numpy(), ref), xcd
    finally:
        eng.set_xcd_remap(-1)


@pytest.mark.parametrize("xcd", [1, 256])
def test_xcd_remap_large_grid(eng, xcd):
    """The XCD orders over a grid large enough that xcd_chunk permutes blocks at the library's
    default grain for big verify batches (K = 256: the first 8 * 256 = 2048 workgroups): 2^16 + 5
    fixed-stride records of 1500 B (98 MB; 8 x 7 emit / verify: 2049 workgroups), corrupted 1 in 7,
    against the oracle over the whole buffer."""
    n, L = (1 << 16) + 5, 1500
    buf = torch.zeros(n * L + 64, dtype=torch.uint8, device="cuda:0")
    batch = E.Batch.fixed(n, L, L, E.KIND_IP)
    eng.synth(buf, batch, E.SYNTH_UDP4, seed=xcd + 77)
    eng.corrupt(buf, batch, every=7, seed=xcd)
    host = buf.cpu().numpy().copy()
    assert (n + 31) // 32 >= 8 * 256  # workgroups of 32 records (G = 8)
    ref_v = oracle.batch_verify(host.copy(), None, n, L, L, E.KIND_IP, CAPS_DEFAULT)
    ref_e = host.copy()
    oracle.batch_emit(ref_e, None, n, L, L, E.KIND_IP, CAPS_DEFAULT)
    eng.set_xcd_remap(xcd)
    try:
        st = eng.verify(buf, batch).cpu().numpy()
        eng.emit(buf, batch)
    finally:
        eng.set_xcd_remap(-1)
    assert np.array_equal(st, ref_v), xcd
    assert np.array_equal(buf.cpu().numpy(), ref_e), xcd


def test_launch_records(eng):
    """Batches split into consecutive launches (smol_csum_tool_set_launch_records): emit, verify
    and data over fixed-stride and descriptor batches, status arrays, copy-emit and 6LoWPAN NHC UDP,
    chunk sizes that do and do not divide the batch, against the oracle and the unsplit launch."""
    rng = np.random.default_rng(17)
    recs = []
    for i in range(1037):
        pl = P.rand_bytes(rng, int(rng.integers(0, 1800)))
        recs.append(P.ipv4(V4A, V4B, 17, P.udp(1000 + i, 53, pl)) if i % 3 else
                    P.ipv6(bytes(16), bytes([1] * 16), 6, P.tcp(1, 2, pl)))
    L = 1500
    n = 2051
    fixed_buf = torch.zeros(n * L + 64, dtype=torch.uint8, device="cuda:0")
    fixed = E.Batch.fixed(n, L, L, E.KIND_IP)
    eng.synth(fixed_buf, fixed, E.SYNTH_UDP4, seed=3)
    eng.corrupt(fixed_buf, fixed, every=9, seed=3)
    host = fixed_buf.cpu().numpy().copy()
    ref_v = oracle.batch_verify(host.copy(), None, n, L, L, E.KIND_IP, CAPS_DEFAULT)
    ref_e = host.copy()
    ref_es = oracle.batch_emit(ref_e, None, n, L, L, E.KIND_IP, CAPS_DEFAULT)
    ref_d = oracle.batch_data(host.copy(), None, n, L, L)
    for per in (1, 7, 256, 1000, 2051, 5000):
        eng.set_launch_records(per)
        try:
            st = eng.verify(fixed_buf, fixed).cpu().numpy()
            d2 = fixed_buf.clone()
            est = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
            eng.emit(d2, fixed, status=est)
            dat = eng.data(fixed_buf, fixed).cpu().numpy()
            _run_records(eng, recs, E.KIND_IP, gap_seed=per)
        finally:
            eng.set_launch_records(0)
        assert np.array_equal(st, ref_v), per
        assert np.array_equal(d2.cpu().numpy(), ref_e), per
        assert np.array_equal(est.cpu().numpy(), ref_es), per
        assert np.array_equal(dat.view(np.uint16), ref_d), per


def test_launch_records_copy_and_nhc(eng):
    """The split launches advance the copy descriptors and the NHC address rows with the records."""
    rng = np.random.default_rng(29)
    n, L = 1029, 1500
    buf = torch.empty(n * L, dtype=torch.uint8, device="cuda:0")
    batch = E.Batch.fixed(n, L, kind=E.KIND_IP)
    eng.synth(buf, batch, E.SYNTH_UDP4, seed=11)
    host = buf.cpu().numpy().copy()
    src = rng.integers(0, 256, n * 1472 + 16, dtype=np.uint8)
    copies = E.make_copies(np.arange(n, dtype=np.uint64) * 1472, 28, 1472)
    ref = host.copy()
    oracle.batch_copy_emit(ref, None, n, src, copies, L, L, E.KIND_IP)
    recs = [P.nhc_udp(rng, i % 4, bool((i >> 2) & 1), int(rng.integers(0, 300))) for i in range(777)]
    nbuf, offs, lens = P.pack(recs, gap_rng=rng)
    addrs = rng.integers(0, 256, (len(recs), 32), dtype=np.uint8)
    nbatch = E.Batch.from_records(offs, lens, E.KIND_RAW, "cuda:0")
    desc = P.oracle_desc(offs, lens, 0)
    ref_nv = oracle.batch_nhc_udp_verify(nbuf.copy(), desc, len(recs), addrs)
    ref_n = nbuf.copy()
    oracle.batch_nhc_udp_emit(ref_n, desc, len(recs), addrs)
    d_addrs = torch.from_numpy(addrs.reshape(-1).copy()).cuda()
    for per in (5, 64, 1000):
        eng.set_launch_records(per)
        try:
            d = torch.from_numpy(host.copy()).cuda()
            eng.copy_emit(d, batch, torch.from_numpy(src).cuda(), torch.from_numpy(copies.view(np.uint8).copy()).cuda())
            got = d.cpu().numpy()
            dn = torch.from_numpy(nbuf.copy()).cuda()
            nst = eng.nhc_udp_verify(dn, nbatch, d_addrs).cpu().numpy()
            eng.nhc_udp_emit(dn, nbatch, d_addrs)
            gotn = dn.cpu().numpy()
        finally:
            eng.set_launch_records(0)
        assert np.array_equal(got, ref), per
        assert np.array_equal(nst, ref_nv), per
        assert np.array_equal(gotn, ref_n), per


def test_dispatch_table_every_row(eng):
    """Every row of the measured fixed-stride dispatch table (csum_api.cpp xwalk_auto,
    dispatch_table.inc, round 6): at each row's first and last length, a length that is not a multiple of
    64 and a gapped stride, emit then verify (1/5 of the records corrupted) with the library's own
    choice, no variant forced, against the oracle; the kernel the table names (kernel_for) is the one
    that ran.  Also the lengths just outside the table (1023, 9024)."""
    rng = np.random.default_rng(64)
    cases = []
    for k in range(125):
        a = 1024 + 64 * k
        cases += [(a, a), (a + 63, a + 63), (a + 28, a + 28), (a + 28, a + 92)]
    cases += [(1023, 1023), (9024, 9024), (9024, 9100)]
    for i, (L, stride) in enumerate(cases):
        n = 19  # two full wavefronts of 8 records and a partial one
        profile = (E.SYNTH_UDP4, E.SYNTH_TCP4, E.SYNTH_V6MIX)[i % 3]
        recs = torch.zeros(n * L + 64, dtype=torch.uint8, device="cuda:0")
        pb = E.Batch.fixed(n, L, L, E.KIND_IP)
        eng.synth(recs, pb, profile, seed=L + i)
        r = recs.cpu().numpy()[: n * L].reshape(n, L)
        host = rng.integers(0, 256, n * stride + 64, dtype=np.uint8)
        for j in range(n):
            host[j * stride: j * stride + L] = r[j]
        batch = E.Batch.fixed(n, stride, L, E.KIND_IP)
        d = torch.from_numpy(host.copy()).cuda()
        want_e = eng.kernel_for("emit", batch)
        eng.emit(d, batch)
        assert eng.last_launch()["kernel"] == want_e, (L, stride)
        ref = host.copy()
        oracle.batch_emit(ref, None, n, stride, L, E.KIND_IP, CAPS_DEFAULT)
        got = d.cpu().numpy()
        assert np.array_equal(got, ref), (L, stride, want_e, np.nonzero(got != ref)[0][:8])
        for j in range(0, n, 5):
            ref[j * stride + int(rng.integers(0, L))] ^= 0x21
        d = torch.from_numpy(ref.copy()).cuda()
        want_v = eng.kernel_for("verify", batch)
        st = eng.verify(d, batch).cpu().numpy()
        assert eng.last_launch()["kernel"] == want_v, (L, stride)
        assert np.array_equal(st, oracle.batch_verify(ref, None, n, stride, L, E.KIND_IP, CAPS_DEFAULT)), (L, stride, want_v)
