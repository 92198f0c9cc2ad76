"""GPU parity of verify_copy (smol_csum_batch_verify_copy): verify's status bytes, each record's payload
span and the payload bytes delivered to the record's slot of a second device buffer, in one pass.

Expected values in every case: the status bytes from the oracle (pktgen.oracle_verify_records), the spans
from tests/test_verify_copy_cpu.py's expected_span (its own restatement of the span rule), and the
destination built in numpy from a buffer filled with the sentinel 0xA5.  The whole destination buffer is
compared, so a stray write anywhere fails.  Each test asserts that the classes it means to exercise occur
in its batch: copied, too big for the cap, no span, malformed, corrupted but delivered.
"""
import os
import subprocess

import numpy as np
import pytest

import oracle
from tests import pktgen as P
from tests.test_verify_copy_cpu import V4A, V4B, V6A, V6B, expected_span

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from smoltcp_amd import engine as E  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xA5
NOCAPS = (0, 0, 0, 0, 0)


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    e = E.ChecksumEngine(0)
    yield e
    e.close()


def _place(recs, offs=None, gap_seed=None, fixed=None):
    """The batch buffer: packed records (random 0..7-byte gaps with gap_seed), records at the given
    offsets, or fixed = (stride, length, base): record i at base + i * stride, padded to `length` bytes with
    random bytes (a record longer than its IP length).  Returns (buf, offs, lens, recs as placed)."""
    rng = np.random.default_rng(77)
    if fixed is not None:
        stride, length, base = fixed
        n = len(recs)
        buf = rng.integers(0, 256, base + n * stride + 16, dtype=np.uint8)
        offs = base + np.arange(n, dtype=np.uint64) * stride
        for i, r in enumerate(recs):
            assert len(r) <= length
            buf[int(offs[i]):int(offs[i]) + len(r)] = np.frombuffer(r, np.uint8)
        placed = [bytes(buf[int(o):int(o) + length]) for o in offs]
        return buf, offs, np.full(n, length, np.uint32), placed
    if offs is not None:
        end = max(int(o) + len(r) for o, r in zip(offs, recs)) if recs else 0
        buf = rng.integers(0, 256, end + 16, dtype=np.uint8)
        for o, r in zip(offs, recs):
            buf[int(o):int(o) + len(r)] = np.frombuffer(r, np.uint8)
        return buf, np.asarray(offs, np.uint64), np.array([len(r) for r in recs], np.uint32), list(recs)
    buf, offs, lens = P.pack(recs, gap_rng=np.random.default_rng(gap_seed) if gap_seed is not None else None)
    return buf, offs, lens, list(recs)


def _slots(spans, rng, policy="mixed", dst_mod=None, dense=False):
    """Destination offsets and caps: slots in shuffled record order, 0..20 random bytes between them
    (dense: none), each slot's start at any alignment (dst_mod[i]: that residue mod 16).  Caps by
    policy: "fit" cap == len, "roomy" len + 0..9, "mixed" also len - 1 and 0 now and then."""
    n = len(spans)
    caps = np.zeros(n, np.uint32)
    for i, sp in enumerate(spans):
        ln = sp[1] if sp else 0
        c = int(rng.integers(0, 10)) if policy == "mixed" else 0
        if policy == "fit" or dense:
            caps[i] = ln
        elif policy == "roomy" or c < 7:
            caps[i] = ln + int(rng.integers(0, 10))
        elif c == 7:
            caps[i] = ln
        elif c == 8:
            caps[i] = max(ln - 1, 0)
        else:
            caps[i] = 0
    offs = np.zeros(n, np.uint64)
    pos = 3
    for i in rng.permutation(n):
        if not dense:
            pos += int(rng.integers(0, 21))
        if dst_mod is not None:
            pos += (int(dst_mod[i]) - pos) % 16
        offs[i] = pos
        pos += int(caps[i])
    return offs, caps, pos + 19


def _run(eng, recs, kinds, rflags=0, caps=NOCAPS, offs=None, gap_seed=1, fixed=None, fill=True, flips=(),
         policy="mixed", dst_mod=None, dense=False, shape=-1, blocks=0, stream=None, seed=0):
    """One verify_copy call, compared exactly.  recs: the packets; kinds / rflags: per record (a
    fixed-stride batch: one value).  fill: the oracle's emit fills every checksum first, then `flips`
    (record, byte offset, bit) corrupt single bits.  Returns the per-record classes."""
    n = len(recs)
    rng = np.random.default_rng(seed)
    kinds_a = np.broadcast_to(np.asarray(kinds, np.uint8), (n,)).copy()
    flags_a = np.broadcast_to(np.asarray(rflags, np.uint8), (n,)).copy()
    buf, offs, lens, placed = _place(recs, offs, gap_seed, fixed)
    desc = E.make_descriptors(offs, lens, kinds_a, flags_a)
    if fill:
        oracle.batch_emit(buf, desc, n)
    for i, o, bit in flips:
        buf[int(offs[i]) + o] ^= 1 << bit
    placed = [bytes(buf[int(o):int(o) + int(ln)]) for o, ln in zip(offs, lens)]
    if flags_a.any():
        ref_st = oracle.batch_verify(buf.copy(), desc, n, caps=caps)
    else:
        ref_st = P.oracle_verify_records(buf.copy(), offs, lens, kinds_a, caps=caps)
    spans = [expected_span(r, int(k), int(f)) for r, k, f in zip(placed, kinds_a, flags_a)]
    d_offs, d_caps, d_size = _slots(spans, rng, policy, dst_mod, dense)
    ref_dst = np.full(d_size, SENTINEL, np.uint8)
    ref_sp = np.zeros(n, E.SPAN_DTYPE)
    for i, sp in enumerate(spans):
        if sp is None:
            continue
        ref_sp[i]["off"], ref_sp[i]["len"] = sp
        if sp[1] <= d_caps[i]:
            ref_sp[i]["copied"] = 1
            ref_dst[int(d_offs[i]):int(d_offs[i]) + sp[1]] = np.frombuffer(placed[i][sp[0]:sp[0] + sp[1]], np.uint8)

    eng.set_shape(shape)
    eng.set_max_blocks(blocks)
    try:
        d = torch.from_numpy(buf.copy()).cuda()
        dst = torch.full((d_size,), SENTINEL, dtype=torch.uint8, device="cuda")
        slots = torch.from_numpy(E.make_slots(d_offs, d_caps).view(np.uint8).copy()).cuda()
        if fixed is not None:
            stride, length, base = fixed
            batch = E.Batch.fixed(n, stride, length, int(kinds_a[0]) if n else E.KIND_IP, flags=int(flags_a[0]) if n else 0)
            dv = d[base:]
        else:
            batch = E.Batch.from_records(offs, lens, kinds_a, "cuda:0", flags=flags_a)
            dv = d
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                st, sp = eng.verify_copy(dv, batch, dst, slots, caps=caps, stream=stream)
            stream.synchronize()
        else:
            st, sp = eng.verify_copy(dv, batch, dst, slots, caps=caps)
        launched = eng.last_launch()
        got_dst, got_st = dst.cpu().numpy(), st.cpu().numpy()
        got_sp = sp.cpu().numpy().reshape(-1).view(E.SPAN_DTYPE)
        assert np.array_equal(d.cpu().numpy(), buf), "the batch buffer is only read"
    finally:
        eng.set_shape(-1)
        eng.set_max_blocks(0)
    if n:
        assert launched["kernel"] == "vcopy_kernel" and launched["variant"] == 0, launched
    assert np.array_equal(got_st, ref_st), np.nonzero(got_st != ref_st)[0][:8]
    bad = np.nonzero(got_sp != ref_sp)[0]
    assert bad.size == 0, f"spans differ at {bad[:8]}: got {got_sp[bad[:4]]} want {ref_sp[bad[:4]]}"
    diff = np.nonzero(got_dst != ref_dst)[0]
    assert diff.size == 0, f"destination bytes differ at {diff[:8]} (got {got_dst[diff[:8]]} want {ref_dst[diff[:8]]})"
    has = np.array([s is not None for s in spans], bool)
    copied = ref_sp["copied"] == 1
    return {"copied": copied, "toobig": has & ~copied, "nospan": ~has,
            "malformed": (ref_st & E.ST_MALFORMED) != 0,
            "delivered_bad": copied & (ref_sp["len"] > 0) & ((ref_st & E.ST_ACCEPT) == 0), "status": ref_st, "spans": ref_sp}


def _packet(rng, i, maxpay=1500):
    kind = i % 6
    pay = P.rand_bytes(rng, int(rng.integers(0, maxpay)))
    if kind == 0:
        return P.ipv4(V4A, V4B, 17, P.udp(1000 + i, 53, pay))
    if kind == 1:
        return P.ipv4(V4A, V4B, 6, P.tcp(2000 + i, 80, pay, doff=5 + i % 3))
    if kind == 2:
        return P.ipv6(V6A, V6B, 6, P.tcp(3000 + i, 443, pay))
    if kind == 3:
        return P.ipv6(V6A, V6B, 17, P.udp(4000 + i, 53, pay))
    if kind == 4:
        return P.ipv4(V4A, V4B, 1, P.icmp_echo(8, pay))
    return P.ipv6(V6A, V6B, 58, P.icmp_echo(128, pay))


def _mixed(rng, n, eth, maxpay=1500):
    """Mixed packets; one in 13 cut short and one in 13 with a bad IP version (malformed), every 7th with
    one bit flipped."""
    recs, flips = [], []
    for i in range(n):
        r = _packet(rng, i, maxpay)
        if eth:
            r = P.eth(r, 0x0800 if r[0] >> 4 == 4 else 0x86DD)
        if i % 13 == 5:
            r = r[:len(r) - 1 - int(rng.integers(0, min(8, len(r) - 1)))]
        elif i % 13 == 6:
            ip = 14 if eth else 0
            r = r[:ip] + bytes([0x10 | r[ip] & 15]) + r[ip + 1:]
        elif i % 7 == 3:
            flips.append((i, int(rng.integers(len(r) // 2, len(r))), int(rng.integers(0, 8))))
        recs.append(r)
    return recs, flips


def _all_classes(c):
    for k in ("copied", "toobig", "nospan", "malformed", "delivered_bad"):
        assert c[k].any(), f"no record of class {k}"


@pytest.mark.parametrize("eth", [False, True])
def test_mixed_records_packed(eng, eth):
    rng = np.random.default_rng(1 + eth)
    recs, flips = _mixed(rng, 1500, eth)
    c = _run(eng, recs, E.KIND_ETH if eth else E.KIND_IP, flips=flips, gap_seed=3, seed=4)
    _all_classes(c)


@pytest.mark.parametrize("eth,stride,length,base", [(False, 1600, 1540, 0), (True, 1571, 1571, 5), (False, 401, 400, 64)])
def test_mixed_records_fixed_stride(eng, eth, stride, length, base):
    rng = np.random.default_rng(stride)
    recs, flips = _mixed(rng, 1100, eth, maxpay=length - 80)
    c = _run(eng, recs, E.KIND_ETH if eth else E.KIND_IP, flips=flips, fixed=(stride, length, base), seed=5)
    _all_classes(c)


def test_all_alignments(eng):
    """Every pair of (payload source address mod 16, destination address mod 16) at the payload lengths
    around one, two and four chunks, and a full-size one."""
    rng = np.random.default_rng(7)
    recs, offs, dmod, pos = [], [], [], 0
    for ln in (1, 15, 16, 17, 31, 33, 63, 64, 65, 100, 1472):
        for sa in range(16):
            for da in range(16):
                r = P.ipv4(V4A, V4B, 17, P.udp(7, 9, P.rand_bytes(rng, ln)))
                pos += (sa - (pos + 28)) % 16  # the device buffers are 16-byte aligned
                offs.append(pos)
                recs.append(r)
                dmod.append(da)
                pos += len(r)
    c = _run(eng, recs, E.KIND_IP, offs=np.array(offs, np.uint64), policy="fit", dst_mod=dmod, seed=8)
    assert c["copied"].all() and len(recs) == 11 * 256
    assert {(int(o) + 28) % 16 for o in offs} == set(range(16))


def test_payload_lengths_and_header_lengths(eng):
    """Empty payloads (UDP length 8, a bare TCP ACK), payloads that start inside the 128-B header window and
    end past it, every TCP data offset and IPv4 IHL, Hop-by-Hop headers that push the payload past the
    window; packed at every record alignment."""
    rng = np.random.default_rng(9)
    recs = []
    for i in range(900):
        m = i % 6
        pay = P.rand_bytes(rng, int(rng.integers(90, 400)))
        if m == 0:
            recs.append(P.ipv4(V4A, V4B, 17, P.udp(7 + i, 9, b"")))
        elif m == 1:
            recs.append(P.ipv4(V4A, V4B, 6, P.tcp(7 + i, 9, b"", flags=0x10)))
        elif m == 2:
            recs.append(P.ipv4(V4A, V4B, 6, P.tcp(7 + i, 9, pay, doff=5 + (i // 6) % 11)))
        elif m == 3:
            ihl = 5 + (i // 6) % 11
            recs.append(P.ipv4(V4A, V4B, 17 if i % 12 == 3 else 6, P.udp(7 + i, 9, pay) if i % 12 == 3 else P.tcp(7 + i, 9, pay),
                               ihl=ihl, options=bytes([1]) * (ihl * 4 - 20)))
        elif m == 4:
            hb = P.hbh(17, 6 + (i // 6) % 34, rng)  # 56 .. 320 B: the UDP header inside, across or past the window
            recs.append(P.ipv6(V6A, V6B, 0, hb + P.udp(7 + i, 9, pay)))
        else:
            hb = P.hbh(6, 4 + (i // 6) % 34, rng)
            recs.append(P.ipv6(V6A, V6B, 0, hb + P.tcp(7 + i, 9, pay, doff=5 + i % 11)))
    c = _run(eng, recs, E.KIND_IP, gap_seed=10, policy="roomy", seed=11)
    assert c["copied"].all()
    sp = c["spans"]
    assert (sp["len"] == 0).sum() >= 300 and (sp["off"] > 128).any() and ((sp["off"] < 128) & (sp["off"] + sp["len"] > 128)).any()
    assert (c["status"] & E.ST_ACCEPT).all()


def test_length_fields_rule_not_the_record_length(eng):
    """A UDP length field shorter than the IP payload (the trailing bytes are neither summed nor
    delivered), and records longer than the IP total length (Ethernet padding to 60 bytes, fixed-stride
    slack)."""
    rng = np.random.default_rng(12)
    recs, kinds = [], []
    for i in range(400):
        pay = P.rand_bytes(rng, 1 + i % 90)
        if i % 2:
            cut = int(rng.integers(0, len(pay)))
            u = P.udp(7 + i, 9, pay)
            u = u[:4] + P.be16(8 + cut) + u[6:]  # the length field ends `cut` bytes into the payload
            recs.append(P.ipv4(V4A, V4B, 17, u))
            kinds.append(E.KIND_IP)
        else:
            f = P.eth(P.ipv4(V4A, V4B, 6 if i % 4 else 17, P.tcp(7 + i, 9, pay[:5]) if i % 4 else P.udp(7 + i, 9, pay[:3])))
            recs.append(f + bytes(max(0, 60 - len(f))) + P.rand_bytes(rng, i % 5))
            kinds.append(E.KIND_ETH)
    c = _run(eng, recs, np.array(kinds, np.uint8), gap_seed=13, policy="fit", seed=14)
    assert c["copied"].all() and (c["status"] & E.ST_ACCEPT).all()
    ends = np.array([len(r) for r in recs]) - (c["spans"]["off"].astype(np.int64) + c["spans"]["len"])
    assert (ends[1::2] > 0).sum() > 150 and (ends[0::2] > 0).sum() > 150  # bytes of the record past the span


@pytest.mark.parametrize("shape", [-1, 0, 7, 1, 8, 4, 6])
def test_long_records_every_shape(eng, shape):
    """1500-, 9000- and 65535-byte IPv4 packets (UDP and TCP, IP and Ethernet records) between short ones,
    at every launch shape of the kernel (8 x 6, 8 x 7, 16 x 3, 16 x 4, 32 x 4, 64 x 4)."""
    rng = np.random.default_rng(15)
    recs, kinds = [], []
    for j, total in enumerate((1500, 9000, 65535, 64, 65535, 9000, 1500, 129, 4097)):
        for udp in (True, False):
            l4 = P.udp(7, 9, P.rand_bytes(rng, total - 28)) if udp else P.tcp(7, 9, P.rand_bytes(rng, total - 40))
            r = P.ipv4(V4A, V4B, 17 if udp else 6, l4)
            assert len(r) == total
            eth = (j + udp) % 2 == 0
            recs.append(P.eth(r) if eth else r)
            kinds.append(E.KIND_ETH if eth else E.KIND_IP)
    flips = [(5, 30000, 3), (9, 65000, 0)]
    c = _run(eng, recs, np.array(kinds, np.uint8), flips=flips, gap_seed=16, policy="roomy", seed=17 + shape, shape=shape)
    assert c["copied"].all() and c["delivered_bad"].any() and c["spans"]["len"].max() == 65535 - 28


def test_cap_decides_the_copy(eng):
    """cap == len copies; cap == len - 1 and cap == 0 do not: copied == 0, the slot untouched, the span
    still reported."""
    rng = np.random.default_rng(18)
    recs = [_packet(rng, i - i % 6 + (0, 1, 2, 3)[i % 4], 700) for i in range(600)]
    c = _run(eng, recs, E.KIND_IP, gap_seed=19, policy="mixed", seed=20)
    assert c["copied"].sum() > 300 and c["toobig"].sum() > 50 and not c["nospan"].any()
    assert (c["spans"]["off"][c["toobig"]] > 0).all() and (c["spans"]["len"][c["toobig"]] > 0).all()


def test_records_without_a_span(eng):
    """Destination port 0, truncated L4, fragments, ICMPv4 / ICMPv6 / IGMP, SMOL_REC_IPHDR_ONLY, the ARP
    ethertype, SMOL_KIND_RAW: off = len = copied = 0 and no byte stored, whatever the cap."""
    rng = np.random.default_rng(21)
    recs, kinds, flags = [], [], []
    for i in range(660):
        pay = P.rand_bytes(rng, 20 + i % 300)
        u4 = P.ipv4(V4A, V4B, 17, P.udp(7 + i, 9, pay))
        m = i % 11
        k, f = E.KIND_IP, 0
        if m == 0:
            r = P.ipv4(V4A, V4B, 17, P.udp(7 + i, 0, pay))
        elif m == 1:
            r = P.ipv4(V4A, V4B, 6, P.tcp(7 + i, 9, pay, doff=8)[:24], total_len=44)
        elif m == 2:
            r = P.ipv4(V4A, V4B, 17, P.udp(7 + i, 9, pay), flags_frag=0x2000 if i % 2 else 0x0020)
        elif m == 3:
            r = P.ipv4(V4A, V4B, 1, P.icmp_echo(8, pay))
        elif m == 4:
            r = P.ipv6(V6A, V6B, 58, P.icmp_echo(128, pay))
        elif m == 5:
            r = P.ipv4(V4A, V4B, 2, bytes([0x11, 0, 0, 0, 224, 0, 0, 1]))
        elif m == 6:
            r, f = u4, E.REC_IPHDR_ONLY
        elif m == 7:
            r, k = P.eth(u4, 0x0806), E.KIND_ETH
        elif m == 8:
            r, k = u4, E.KIND_RAW
        elif m == 9:
            r = P.ipv6(V6A, V6B, 6, P.tcp(0, 9, pay))
        else:
            r = u4  # a good record between them
        recs.append(r)
        kinds.append(k)
        flags.append(f)
    c = _run(eng, recs, np.array(kinds, np.uint8), np.array(flags, np.uint8), gap_seed=22, policy="roomy", seed=23)
    assert c["nospan"].sum() == 600 and c["copied"].sum() == 60 and c["malformed"].sum() >= 150
    assert not c["spans"]["off"][c["nospan"]].any() and not c["spans"]["len"][c["nospan"]].any()


def test_corrupted_records_are_delivered_as_they_stand(eng):
    """One flipped bit in the payload, the L4 header or an IP address: the status lacks ACCEPT, and the
    payload arrives exactly as it stands in the buffer."""
    rng = np.random.default_rng(24)
    recs, flips = [], []
    for i in range(600):
        r = _packet(rng, i - i % 6 + (0, 1, 2, 3)[i % 4], 900)
        sp = expected_span(r, E.KIND_IP)
        recs.append(r)
        where = i % 3
        if where == 0 and sp[1]:
            flips.append((i, sp[0] + int(rng.integers(0, sp[1])), int(rng.integers(0, 8))))
        elif where == 1:
            flips.append((i, (16 if r[0] >> 4 == 4 else 30), int(rng.integers(0, 8))))  # an address byte
    c = _run(eng, recs, E.KIND_IP, flips=flips, gap_seed=25, policy="roomy", seed=26)
    hit = np.zeros(len(recs), bool)
    hit[[f[0] for f in flips]] = True
    assert c["copied"].all() and not (c["status"][hit] & E.ST_ACCEPT).any() and (c["status"][~hit] & E.ST_ACCEPT).all()
    assert c["delivered_bad"].sum() > 300


def test_every_caps_combination_equals_verify(eng):
    rng = np.random.default_rng(27)
    recs, flips = _mixed(rng, 240, False, maxpay=300)
    buf, offs, lens, _ = _place(recs, gap_seed=28)
    kinds = np.ones(len(recs), np.uint8)
    oracle.batch_emit(buf, E.make_descriptors(offs, lens, kinds), len(recs))
    for i, o, bit in flips:
        buf[int(offs[i]) + o] ^= 1 << bit
    d = torch.from_numpy(buf).cuda()
    batch = E.Batch.from_records(offs, lens, kinds, "cuda:0")
    slots = torch.from_numpy(E.make_slots(np.arange(len(recs), dtype=np.uint64) * 1500, 1500).view(np.uint8).copy()).cuda()
    dst = torch.full((len(recs) * 1500,), SENTINEL, dtype=torch.uint8, device="cuda")
    first_dst = first_sp = None
    seen = set()
    for code in range(4 ** 5):
        caps = tuple((code >> (2 * j)) & 3 for j in range(5))
        st, sp = eng.verify_copy(d, batch, dst, slots, caps=caps)
        assert torch.equal(st, eng.verify(d, batch, caps=caps)), caps
        seen.add(bytes(st.cpu().numpy()))
        if first_dst is None:
            first_dst, first_sp = dst.clone(), sp.clone()
        elif code % 97 == 0:  # the caps touch neither the spans nor the copy
            assert torch.equal(dst, first_dst) and torch.equal(sp, first_sp)
    assert len(seen) > 8  # the caps did change the verdicts


def test_dense_slots_share_segments(eng):
    """Thousands of 1- to 40-byte payloads delivered back to back in shuffled record order, so that many
    slots share every 64-B segment and neighbouring slots are written by other wavefronts: byte-masked
    stores, no read-modify-write.  Run once, compared exactly."""
    rng = np.random.default_rng(29)
    recs = []
    for i in range(6000):
        pay = P.rand_bytes(rng, int(rng.integers(1, 41)))
        recs.append(P.ipv4(V4A, V4B, 17, P.udp(7, 9, pay)) if i % 2 else P.ipv6(V6A, V6B, 6, P.tcp(7, 9, pay)))
    c = _run(eng, recs, E.KIND_IP, gap_seed=30, dense=True, seed=31)
    assert c["copied"].all() and (c["status"] & E.ST_ACCEPT).all()


def test_batch_sizes_grid_wrap_and_stream(eng):
    rng = np.random.default_rng(32)
    small = [P.ipv4(V4A, V4B, 17, P.udp(7 + i % 100, 9, P.rand_bytes(rng, 36))) for i in range(5000)]
    assert len(small[0]) == 64
    _run(eng, [], E.KIND_IP, fill=False)                      # n = 0: nothing launched
    c = _run(eng, small[:1], E.KIND_IP, policy="fit", seed=33)  # n = 1
    assert c["copied"].all()
    # 3 workgroups of 32 groups each: the grid-stride loop wraps 52 times
    c = _run(eng, small, E.KIND_IP, fixed=(64, 64, 0), blocks=3, policy="roomy", seed=34)
    assert c["copied"].all()
    c = _run(eng, small[:700], E.KIND_IP, gap_seed=35, blocks=2, seed=36)  # the same over descriptors
    assert c["copied"].any() and c["toobig"].any()
    c = _run(eng, small[:300], E.KIND_IP, gap_seed=37, stream=torch.cuda.Stream(), seed=38)
    assert c["copied"].any()


def test_empty_batch_launches_nothing(eng):
    e = torch.zeros(16, dtype=torch.uint8, device="cuda")
    st, sp = eng.verify_copy(e, E.Batch.fixed(0, 64, 64, E.KIND_IP), e, e)
    assert st.numel() == 0 and sp.numel() == 0
    with pytest.raises(Exception):
        eng.verify_copy(e, E.Batch.fixed(1, 16, 16, E.KIND_IP), e, torch.zeros(32, dtype=torch.uint8, device="cuda")[8:24])


def test_rx_split_tool():
    """tools/rx_split: a few thousand Ethernet frames through Engine::verify_copy into a dense payload
    arena, checked against its own slicing of the frames and against Engine::verify."""
    assert torch.cuda.is_available()
    tools = os.path.join(ROOT, "tools")
    subprocess.run(["make", "-s", "-C", tools, "rx_split"], check=True)
    r = subprocess.run([os.path.join(tools, "rx_split")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rx_split ok" in r.stdout
