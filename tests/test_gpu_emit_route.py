"""GPU: the two-launch route of fixed-stride whole-segment emit (the fields-sink kernel into the context's
entries, then the segment pass: csrc/csum_api.cpp run_one(), csrc/csum_segpass.hip) against the CPU oracle.

Every case runs smol_csum_batch_emit with the route forced on (set_emit_route(1)) and compares the WHOLE
tensor, 128 random guard bytes on each side, the bytes between the tensor's start and the batch, the
records past the batch's last and every gap byte included, byte for byte with oracle.batch_emit, and with
torch.equal against the same call with the route off; the status bytes likewise (8 bytes past n stay as
they were).  The oracle runs once per batch layout and is shared by the record counts and placements.
A length whose dispatch-table row is not a whole-segment transposed-walk emit (variants 101 / 57) keeps
one launch also when the route is forced on: the comparison holds all the same, and last_route says which
it was (smol_csum_tool_pick names the row's kernel)."""
import ctypes

import numpy as np
import pytest

import oracle
from tests import pktgen as P

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from smoltcp_amd import _lib  # noqa: E402
from smoltcp_amd import engine as E  # noqa: E402

CAPS_DEFAULT = (0, 0, 0, 0, 0)
# the automatic route (csum_api.cpp kRouteMinRecords / kRouteMaxRecords and the length range): the measured decision
AUTO_ROUTE, AUTO_MIN_RECORDS, AUTO_MAX_RECORDS = True, 1 << 20, 1 << 21
GUARD = 128
NMAX = 100
COUNTS = (1, 7, 8, 9, 19, 33, 100)  # a partial wavefront, lane-group seams of the pass, K = 4 not dividing n
PLACES = (0, 4, 36, 60)             # the batch's start modulo 64: record 0's segment would start before the batch
# (length, stride): the transposed walk at R = 8 up to 1921 B and at R = 4 from 1922 B; 1500 at stride 1564
# is the gapped stride of the issue (its row runs the walk kernel: one launch), 1100 at 1164 a gapped
# stride whose row does take the route
LAYOUTS = [(1024, 1024), (1087, 1087), (1472, 1472), (1500, 1500), (1536, 1536), (1921, 1921), (1922, 1922),
           (1500, 1564), (1100, 1164)]
PROFILES = [E.SYNTH_UDP4, E.SYNTH_TCP4, E.SYNTH_V6MIX]
V4A, V4B = bytes([10, 0, 0, 1]), bytes([10, 0, 0, 2])
V6A, V6B = bytes(range(16)), bytes(range(16, 32))


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    e = E.ChecksumEngine(0)
    yield e
    e.close()


def _route_row(length, stride, n=NMAX, flags=0):
    """Whether pick_kernel answers a whole-segment transposed-walk emit (variants 101 / 57) for the batch."""
    L = _lib.lib()
    b = E.Batch.fixed(n, stride, length, E.KIND_IP, flags=flags).c()
    out = (ctypes.c_int32 * 3)()
    assert L.smol_csum_tool_pick(-1, -1, 1, 1, ctypes.byref(b), 0, out) == 0
    return out[0] == 2 and out[1] in (101, 57)


def _force_zero_udp4(rec: bytes) -> bytes:
    """Adjust one payload word of an IPv4/UDP packet so that its computed UDP checksum becomes 0."""
    buf, offs, lens = P.pack([rec])
    P.oracle_emit_records(buf, offs, lens, E.KIND_IP)
    c = int(buf[26]) << 8 | int(buf[27])
    b = bytearray(rec)
    w = (b[28] << 8 | b[29]) + c
    w = (w & 0xFFFF) + (w >> 16)
    b[28], b[29] = w >> 8, w & 0xFF
    return bytes(b)


def _hand_records(rng, L):
    """Records of exactly L bytes that the synthetic profiles do not hold."""
    pl = lambda k: P.rand_bytes(rng, L - k)  # noqa: E731
    inner = P.ipv4(V4B, V4A, 17, P.rand_bytes(rng, L - 48), csum=0x1234)
    lies = bytearray(P.ipv4(V4A, V4B, 17, P.udp(1, 2, pl(28))))
    lies[2], lies[3] = 0xFF, 0xFF  # total length past the record
    udp_lies = bytearray(P.ipv4(V4A, V4B, 17, P.udp(1, 2, pl(28))))
    udp_lies[24], udp_lies[25] = 0xFF, 0xFF  # UDP length past the datagram
    noip = bytearray(P.ipv4(V4A, V4B, 17, P.udp(1, 2, pl(28))))
    noip[0] = 0x35  # no IP version: no field at all
    recs = [
        P.ipv4(V4A, V4B, 6, P.tcp(7, 9, pl(80)), ihl=15, options=P.rand_bytes(rng, 40)),  # fields at 10 and 76
        P.ipv4(V4A, V4B, 17, P.udp(7, 9, pl(52)), ihl=11, options=P.rand_bytes(rng, 24)),
        P.ipv4(V4A, V4B, 1, P.icmp4_error(3, 1, inner, csum=0xBEEF)),  # a third field (the inner header's)
        P.ipv6(V6A, V6B, 0, P.hbh(17, 32, rng) + P.udp(3, 4, pl(40 + 264 + 8))),  # L4 field at 310: past the window
        P.ipv6(V6A, V6B, 0, P.hbh(6, 8, rng) + P.tcp(3, 4, pl(40 + 72 + 20))),  # at 128: the window's edge
        _force_zero_udp4(P.ipv4(V4A, V4B, 17, P.udp(5, 6, pl(28)))),  # computes to 0: sent as 0xffff
        bytes(noip), bytes(lies), bytes(udp_lies),
        P.ipv4(V4A, V4B, 47, pl(20)),  # a protocol without an L4 checksum: the header's field only
        P.ipv4(V4A, V4B, 1, P.icmp_echo(8, pl(28))),
        P.ipv4(V4A, V4B, 17, P.udp(1, 2, pl(28)), flags_frag=0x2000),  # a fragment: header only
    ]
    assert all(len(r) == L for r in recs), [len(r) for r in recs]
    return recs


HAND_AT = (1, 2, 3, 4, 5, 6, 8, 10, 12, 17, 18, 32)  # some in every record count above 1, and at lane-group seams


class Layout:
    """NMAX records of one (length, stride, profile), hand-built ones among them, and the oracle's emit of them
    (computed once); tensor(place) lays them out behind the guard at a start address of `place` modulo 64."""

    def __init__(self, eng, length, stride, profile, caps=CAPS_DEFAULT, flags=0, seed=1):
        self.length, self.stride, self.caps, self.flags = length, stride, caps, flags
        rng = np.random.default_rng(seed * 7919 + length)
        t = torch.from_numpy(rng.integers(0, 256, NMAX * stride, dtype=np.uint8)).to("cuda:0")  # random gap bytes
        eng.synth(t, E.Batch.fixed(NMAX, stride, length, E.KIND_IP), profile, seed=seed + length)
        self.body = t.cpu().numpy()
        for i, r in zip(HAND_AT, _hand_records(rng, length)):
            self.body[i * stride:i * stride + length] = np.frombuffer(r, np.uint8)
        self.emitted = self.body.copy()
        self.status = oracle.batch_emit(self.emitted, None, NMAX, stride, length, oracle.kind_flags(E.KIND_IP, flags), caps)
        self.rng = rng

    def tensor(self, place, n):
        """(the whole tensor before the call, the expected whole tensor, the batch's first byte in it)."""
        pre = self.rng.integers(0, 256, GUARD + place, dtype=np.uint8)
        post = self.rng.integers(0, 256, GUARD, dtype=np.uint8)
        before = np.concatenate([pre, self.body, post])
        want = before.copy()
        start = GUARD + place
        want[start:start + n * self.stride] = self.emitted[:n * self.stride]
        return torch.from_numpy(before).to("cuda:0"), torch.from_numpy(want).to("cuda:0"), start


def _emit(eng, whole, start, lay: Layout, n, route, status=True, stream=None, chunk=0):
    """One emit of the first n records in a clone of `whole`; returns (the tensor, status or None, last_route)."""
    buf = whole.clone()
    assert buf.data_ptr() % 256 == 0
    view = buf[start:start + NMAX * lay.stride]
    st = torch.full((n + 8,), 0xA5, dtype=torch.uint8, device="cuda:0") if status else None
    eng.set_emit_route(route)
    eng.set_route_chunk(chunk)
    try:
        eng.emit(view, E.Batch.fixed(n, lay.stride, lay.length, E.KIND_IP, flags=lay.flags), caps=lay.caps, status=st,
                 stream=stream)
        took = eng.last_route()
        launched = eng.last_launch()
    finally:
        eng.set_emit_route(-1)
        eng.set_route_chunk(0)
    return buf, st, took, launched


def _check(eng, lay: Layout, n, place, chunk=0, status=True, tag=""):
    whole, want, start = lay.tensor(place, n)
    row = _route_row(lay.length, lay.stride, n, lay.flags)
    on, st_on, took, launched = _emit(eng, whole, start, lay, n, 1, status, chunk=chunk)
    off, st_off, took_off, launched_off = _emit(eng, whole, start, lay, n, 0, status)
    torch.cuda.synchronize()
    where = (tag, lay.length, lay.stride, n, place, chunk)
    assert took == row and not took_off, (where, took, took_off, row)
    assert launched == launched_off, (where, launched, launched_off)  # the launch record is the picked kernel's
    if not torch.equal(on, want):
        bad = torch.nonzero(on != want).flatten()[:8].cpu().numpy() - start
        raise AssertionError((where, "route on differs from the oracle at batch offsets", bad, bad % lay.stride))
    assert torch.equal(off, want), (where, "route off differs from the oracle")
    assert torch.equal(on, off), where
    if status:
        ref = np.concatenate([lay.status[:n], np.full(8, 0xA5, np.uint8)])
        assert np.array_equal(st_on.cpu().numpy(), ref), (where, "status, route on")
        assert torch.equal(st_on, st_off), (where, "status")


@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("length,stride", LAYOUTS)
def test_route_matches_oracle(eng, length, stride, profile):
    lay = Layout(eng, length, stride, profile)
    for n in COUNTS:
        for place in PLACES:
            _check(eng, lay, n, place, status=(n + place) % 2 == 0)
    assert _route_row(1500, 1500) and _route_row(1100, 1164) and _route_row(1922, 1922)


def test_chunk_seams(eng):
    """Chunks of 16 records in a 100-record batch (and of 7: seams off the lane groups' grid)."""
    for length, stride in ((1500, 1500), (1087, 1087), (1100, 1164)):
        lay = Layout(eng, length, stride, E.SYNTH_V6MIX, seed=5)
        for chunk in (16, 7):
            for place in (0, 36):
                _check(eng, lay, NMAX, place, chunk=chunk, tag="chunk")


def test_caps_and_header_only(eng):
    """Every checksum None / ignored on send in turn, all of them, and SMOL_REC_IPHDR_ONLY records."""
    combos = [tuple(c if j == i else 0 for j in range(5)) for i in range(5) for c in (1, 3)] + [(3,) * 5]
    for caps in combos:
        lay = Layout(eng, 1500, 1500, E.SYNTH_V6MIX, caps=caps, seed=9)
        _check(eng, lay, 33, 4, tag=("caps", caps))
    for profile in (E.SYNTH_UDP4, E.SYNTH_V6MIX):
        lay = Layout(eng, 1500, 1500, profile, flags=E.REC_IPHDR_ONLY, seed=11)
        _check(eng, lay, 33, 36, tag="iphdr-only")
        _check(eng, lay, NMAX, 0, chunk=16, tag="iphdr-only")


def test_two_streams(eng):
    """Emits of two buffers alternate on two streams of one context with nothing ordering them: both match
    the oracle (the entries are the context's; a call on another stream waits for the previous one)."""
    la, lb = Layout(eng, 1500, 1500, E.SYNTH_UDP4, seed=21), Layout(eng, 1087, 1087, E.SYNTH_V6MIX, seed=22)
    wa, want_a, sa = la.tensor(4, NMAX)
    wb, want_b, sb = lb.tensor(60, NMAX)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    bufs = [(wa.clone(), wb.clone()) for _ in range(6)]
    ba, bb = E.Batch.fixed(NMAX, la.stride, la.length, E.KIND_IP), E.Batch.fixed(NMAX, lb.stride, lb.length, E.KIND_IP)
    torch.cuda.synchronize()  # the buffers are ready; nothing orders the calls below
    eng.set_emit_route(1)
    try:
        for a, b in bufs:
            eng.emit(a[sa:sa + NMAX * la.stride], ba, stream=s1)
            assert eng.last_route()
            eng.emit(b[sb:sb + NMAX * lb.stride], bb, stream=s2)
            assert eng.last_route()
    finally:
        eng.set_emit_route(-1)
    torch.cuda.synchronize()
    for a, b in bufs:
        assert torch.equal(a, want_a) and torch.equal(b, want_b)


def test_launch_records_across_route(eng):
    """launch_records 40 over 100 records: sub-batches of 40, 40 and 20, each with its own choice of kernel and
    its own route chunks (16: seams at 16, 32 and 40 inside each).  Bytes and status against the oracle and the
    route-off run (which goes out as three launches too); last_route reports the last sub-batch."""
    eng.set_launch_records(40)
    try:
        for length, stride in ((1500, 1500), (1100, 1164)):
            assert _route_row(length, stride, 40) and _route_row(length, stride, 20)
            lay = Layout(eng, length, stride, E.SYNTH_V6MIX, seed=41)
            for place in (0, 36):
                _check(eng, lay, NMAX, place, chunk=16, tag="launch_records")  # (asserts last_route with the route on)
    finally:
        eng.set_launch_records(0)


def test_two_scratch_users_two_streams(eng):
    """The entry buffer's two users, the staged descriptor emit (variant 97, forced: it takes no sample) and
    the fixed-stride route, alternate on two streams of one context with nothing ordering them, the streams
    swapped in odd rounds: every buffer matches the oracle's emit."""
    la, lb = Layout(eng, 1087, 1087, E.SYNTH_V6MIX, seed=51), Layout(eng, 1500, 1500, E.SYNTH_UDP4, seed=52)
    wa, want_a, sa = la.tensor(60, NMAX)
    wb, want_b, sb = lb.tensor(4, NMAX)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    bufs = [(wa.clone(), wb.clone()) for _ in range(6)]
    offs = np.arange(NMAX, dtype=np.uint64) * la.stride
    ba = E.Batch.from_records(offs, np.full(NMAX, la.length), E.KIND_IP, "cuda:0")
    bb = E.Batch.fixed(NMAX, lb.stride, lb.length, E.KIND_IP)
    torch.cuda.synchronize()  # the buffers and descriptors are ready; nothing orders the calls below
    eng.set_emit_route(1)
    try:
        for r, (a, b) in enumerate(bufs):
            first, second = (s1, s2) if r % 2 == 0 else (s2, s1)
            eng.set_variant(97)
            eng.emit(a[sa:sa + NMAX * la.stride], ba, stream=first)
            launched = eng.last_launch()
            assert launched["kernel"] == "dwalk_kernel" and launched["variant"] == 97 and not eng.last_route(), (r, launched)
            eng.set_variant(-1)
            eng.emit(b[sb:sb + NMAX * lb.stride], bb, stream=second)
            assert eng.last_route(), r
    finally:
        eng.set_variant(-1)
        eng.set_emit_route(-1)
    torch.cuda.synchronize()
    for r, (a, b) in enumerate(bufs):
        assert torch.equal(a, want_a), (r, "staged descriptor emit")
        assert torch.equal(b, want_b), (r, "route")


def test_capture_keeps_one_launch(eng):
    """An eager emit (the pair), then one emit captured with torch.cuda.graph: a linear graph of the
    one-launch form, replayed twice on fresh input."""
    lay = Layout(eng, 1500, 1500, E.SYNTH_TCP4, seed=31)
    whole, want, start = lay.tensor(36, NMAX)
    eager, _, took, _ = _emit(eng, whole, start, lay, NMAX, 1, status=False)
    assert took
    buf = whole.clone()
    view = buf[start:start + NMAX * lay.stride]
    batch = E.Batch.fixed(NMAX, lay.stride, lay.length, E.KIND_IP)
    eng.set_emit_route(1)
    try:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                eng.emit(view, batch, stream=s)
        assert not eng.last_route(), "a captured emit took the pair"
    finally:
        eng.set_emit_route(-1)
    for _ in range(2):
        buf.copy_(whole)  # fresh input
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(buf, want)
    assert torch.equal(eager, want)


def test_automatic_route(eng):
    """The automatic route is on for a C2-shaped batch at the library's least batch and above (up to the
    largest batch it won at), and off below it, at a length outside its range, with a forced variant, with
    descriptors and with SMOL_BATCH_FIELD_STORES."""
    n, L = AUTO_MIN_RECORDS, 1500
    buf = torch.zeros(n * L, dtype=torch.uint8, device="cuda:0")
    batch = E.Batch.fixed(n, L, L, E.KIND_IP)
    eng.synth(buf, batch, E.SYNTH_UDP4, seed=3)
    host = buf.cpu().numpy().copy()
    oracle.batch_emit(host, None, n, L, L, E.KIND_IP, CAPS_DEFAULT)
    eng.emit(buf, batch)
    assert eng.last_route() == AUTO_ROUTE
    assert np.array_equal(buf.cpu().numpy(), host)
    eng.emit(buf, E.Batch.fixed(n - 1, L, L, E.KIND_IP))
    assert not eng.last_route()
    big = torch.zeros((AUTO_MAX_RECORDS + 1) * L, dtype=torch.uint8, device="cuda:0")  # (no IP version: nothing to write)
    eng.emit(big, E.Batch.fixed(n, 1400, 1400, E.KIND_IP))  # a length outside the range
    assert not eng.last_route()
    eng.emit(big, E.Batch.fixed(AUTO_MAX_RECORDS, L, L, E.KIND_IP))
    assert eng.last_route() == AUTO_ROUTE
    eng.emit(big, E.Batch.fixed(AUTO_MAX_RECORDS + 1, L, L, E.KIND_IP))
    assert not eng.last_route()
    del big
    eng.set_emit_route(1)
    try:
        eng.set_variant(101)
        eng.emit(buf, batch)
        assert not eng.last_route(), "a forced variant runs its registered form"
        eng.set_variant(-1)
        eng.emit(buf, E.Batch.fixed(n, L, L, E.KIND_IP, flags=E.BATCH_FIELD_STORES))
        assert not eng.last_route()
        offs = np.arange(256, dtype=np.uint64) * L
        eng.emit(buf, E.Batch.from_records(offs, np.full(256, L), E.KIND_IP, "cuda:0"))
        assert not eng.last_route()
        eng.emit(buf, batch)
        assert eng.last_route()
    finally:
        eng.set_variant(-1)
        eng.set_emit_route(-1)
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy(), host)  # emit of an emitted batch changes nothing
