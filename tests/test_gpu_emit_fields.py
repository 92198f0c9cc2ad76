"""GPU: smol_csum_batch_emit_fields against the CPU oracle.

Every case checks, for each kernel form that serves the batch (the library's choice and each forced
form, named by last_launch):
  1. the device buffer is bit-identical before and after the call, gap bytes and 256 guard bytes on
     each side included;
  2. the entries applied to a host copy (engine.apply_fields) equal oracle.batch_emit of that copy,
     byte for byte;
  3. each entry's status is the status byte emit reports per the oracle;
  4. unused slots are off = 0xffff, val = 0, and reserved is 0;
  5. eight extra entries past n, prefilled with 0xA5, are untouched.
The oracle's result is computed once per batch and shared by the forms."""
import numpy as np
import pytest

import oracle
from tests import pktgen as P

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from smoltcp_amd import _lib  # noqa: E402
from smoltcp_amd import engine as E  # noqa: E402

CAPS_DEFAULT = (0, 0, 0, 0, 0)
GUARD = 256
AUTO, WALK, XWALK, DWALK = 0, 1, 2, 3
KERNEL = {WALK: "csum_fields_kernel", XWALK: "xwalk_kernel(fields)", DWALK: "dwalk_kernel(fields)"}
V4A, V4B = bytes([10, 0, 0, 1]), bytes([10, 0, 0, 2])


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    e = E.ChecksumEngine(0)
    yield e
    e.close()


def _guarded(host: np.ndarray):
    """The device copy of `host` between two guard regions; returns (whole tensor, the view of host)."""
    g = np.full(GUARD, 0xC3, dtype=np.uint8)
    whole = torch.from_numpy(np.concatenate([g, host, g])).to("cuda:0")
    return whole, whole[GUARD:GUARD + host.size]


class Ref:
    """The oracle's emit of one batch under `caps`: the emitted host copy and the status bytes."""

    def __init__(self, host, desc, n, stride, length, kind, caps):
        self.host, self.desc, self.n = host, desc, n
        self.emitted = host.copy()
        self.status = oracle.batch_emit(self.emitted, desc, n, stride, length, kind, caps)
        if desc is not None:
            self.offs, self.lens = desc["offset"].astype(np.int64), desc["len"].astype(np.int64)
        else:
            self.offs, self.lens = np.arange(n, dtype=np.int64) * stride, np.full(n, length, dtype=np.int64)


def _prepare(whole, n):
    """A copy of the device buffer to compare with, and n + 8 entries prefilled with 0xA5."""
    return whole.clone(), torch.full((n + 8, 16), 0xA5, dtype=torch.uint8, device="cuda:0")


def _launch(eng, view, batch, caps, forced, want_kernel, ent, stream=None, tag=""):
    eng.set_fields_kernel(forced)
    try:
        out = eng.emit_fields(view, batch, caps=caps, fields=ent, stream=stream)
        launched = eng.last_launch()
    finally:
        eng.set_fields_kernel(AUTO)
    assert out is ent
    if want_kernel is not None and batch.n:
        assert launched["kernel"] == want_kernel, (tag, forced, launched)


def _check(eng, whole, view, batch, ref: Ref, caps, forced, want_kernel, tag=""):
    before, ent = _prepare(whole, ref.n)
    _launch(eng, view, batch, caps, forced, want_kernel, ent, tag=tag)
    torch.cuda.synchronize()
    return _compare(whole, before, ent, ref, tag, forced)


def _compare(whole, before, ent, ref: Ref, tag, forced):
    n = ref.n
    assert torch.equal(whole, before), (tag, forced, "the device buffer changed")  # 1
    e = ent.cpu().numpy()
    assert (e[n:] == 0xA5).all(), (tag, forced, "entries past n written")  # 5
    f = e[:n].reshape(-1).view(E.FIELDS_DTYPE)
    patched = ref.host.copy()
    ok = E.apply_fields(patched, ref.offs, ref.lens, f)
    assert ok.all(), (tag, forced, "a field outside its record", np.flatnonzero(~ok)[:8])
    diff = np.flatnonzero(patched != ref.emitted)
    assert diff.size == 0, (tag, forced, "patched bytes differ from the oracle's emit at", diff[:8])  # 2
    bad = np.flatnonzero(f["status"] != ref.status)
    assert bad.size == 0, (tag, forced, "status", bad[:8], f["status"][bad[:8]], ref.status[bad[:8]])  # 3
    none = f["off"] == _lib.NO_FIELD
    assert (f["val"][none] == 0).all() and not f["reserved"].any(), (tag, forced)  # 4
    return f


# ---------------------------------------------------------------------------------------------
# Fixed stride
# ---------------------------------------------------------------------------------------------

# short records; the transposed walk's first length (1024: forced only) and the dispatch threshold
# (1279 / 1280); its records-per-wavefront boundaries (1921 / 1922, 3969 / 3970, 8065 / 8066); past
# verify's table (9024); its last length and the first one past it (16257 / 16258)
LENGTHS = [64, 1000, 1023, 1024, 1279, 1280, 1500, 1921, 1922, 3969, 3970, 8065, 8066, 9024, 16257, 16258]
XWALK_FIRST, XWALK_AUTO_FIRST, XWALK_LAST = 1024, 1280, 16257
PROFILES = [(E.SYNTH_UDP4, E.KIND_IP), (E.SYNTH_V6MIX, E.KIND_IP), (E.SYNTH_ETH_TCP4, E.KIND_ETH)]


def _auto_kernel(length, stride):
    """csum_dispatch.h pick_fields: the transposed walk from 1280 B up to its last length."""
    return KERNEL[XWALK] if XWALK_AUTO_FIRST <= length <= XWALK_LAST else KERNEL[WALK]


def _fixed_case(eng, profile, kind, n, length, stride, seed, tag):
    host_t = torch.zeros(n * stride + 16, dtype=torch.uint8, device="cuda:0")
    # gap bytes that are not zero, then the records
    host_t[:] = torch.arange(host_t.numel(), device="cuda:0").to(torch.uint8) | 1
    batch = E.Batch.fixed(n, stride, length, kind)
    eng.synth(host_t, batch, profile, seed=seed)
    host = host_t.cpu().numpy()
    whole, view = _guarded(host)
    ref = Ref(host, None, n, stride, length, kind, CAPS_DEFAULT)
    forms = [(AUTO, _auto_kernel(length, stride)), (WALK, KERNEL[WALK])]
    # a forced form that does not fit gives way to the walk kernel
    forms.append((XWALK, KERNEL[XWALK] if XWALK_FIRST <= length <= XWALK_LAST else KERNEL[WALK]))
    forms.append((DWALK, KERNEL[WALK]))  # descriptor batches only
    for forced, want in forms:
        _check(eng, whole, view, batch, ref, CAPS_DEFAULT, forced, want, tag=(tag, length, stride, n))


@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("profile,kind", PROFILES)
def test_fixed_stride(eng, profile, kind, length):
    for stride in (length, length + 64):
        _fixed_case(eng, profile, kind, 1021, length, stride, seed=length * 3 + stride, tag="fixed")


@pytest.mark.parametrize("profile,kind", PROFILES)
def test_fixed_stride_odd_starts_and_tiny_batches(eng, profile, kind):
    _fixed_case(eng, profile, kind, 1021, 1500, 1501, seed=77, tag="odd")  # odd record starts
    _fixed_case(eng, profile, kind, 1021, 1000, 1001, seed=78, tag="odd")
    for n in (1, 7):
        for length in (64, 1279, 1500, 3970, 9024):
            _fixed_case(eng, profile, kind, n, length, length, seed=n * 100 + length, tag="tiny")


# ---------------------------------------------------------------------------------------------
# Descriptor batches
# ---------------------------------------------------------------------------------------------


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


def _mixed_records(rng, n):
    """(records, kinds, flags): IP and Ethernet records of 64-9000 B covering every field layout emit
    has, and the records it leaves alone."""
    recs, kinds, flags = [], [], []
    for i in range(n):
        # payload length: mostly MTU-sized and below, a share of jumbo frames
        pl_len = int(rng.integers(36, 1440)) if i % 4 else int(rng.integers(1440, 8900))
        pl = P.rand_bytes(rng, pl_len)
        s4, d4 = P.rand_bytes(rng, 4), P.rand_bytes(rng, 4)
        s6, d6 = P.rand_bytes(rng, 16), P.rand_bytes(rng, 16)
        t = i % 16
        v6 = False
        if t == 0:
            r = P.ipv4(s4, d4, 17, P.udp(7, 9, pl))
        elif t == 1:
            r = P.ipv4(s4, d4, 6, P.tcp(7, 9, pl), ihl=5 + i % 11, options=P.rand_bytes(rng, (i % 11) * 4))
        elif t == 2:
            r, v6 = P.ipv6(s6, d6, 17, P.udp(7, 9, pl)), True
        elif t == 3:
            r, v6 = P.ipv6(s6, d6, 6, P.tcp(7, 9, pl, doff=5 + i % 6)), True
        elif t == 4:  # ICMPv4 DstUnreachable / TimeExceeded: the embedded header is the third field
            inner = P.ipv4(d4, s4, 17, P.rand_bytes(rng, 8 + i % 64), ihl=5 + i % 3, options=bytes((i % 3) * 4),
                           csum=int(rng.integers(0, 65536)))
            r = P.ipv4(s4, d4, 1, P.icmp4_error(3 if i % 32 < 16 else 11, i % 5, inner, csum=0xBEEF))
        elif t == 5:
            r = P.ipv4(s4, d4, 1, P.icmp_echo(8, pl))
        elif t == 6:
            r, v6 = P.ipv6(s6, d6, 58, P.icmp6(128 + i % 2, 4 + pl_len % 300, rng)), True
        elif t == 7:  # IGMP: always filled
            r = P.ipv4(s4, d4, 2, bytes([0x16, 0, 0xAA, 0x55]) + P.rand_bytes(rng, 4))
        elif t == 8:  # UDP whose checksum computes to 0: sent as 0xffff
            r = _force_zero_udp4(P.ipv4(V4A, V4B, 17, P.udp(5, 6, P.rand_bytes(rng, 2 * (8 + i % 40)))))
        elif t == 9:  # a Hop-by-Hop header of 264 .. 2048 B: the L4 field past the 256-B LDS window
            units = [32, 60, 128, 255][(i // 16) % 4]
            nh = [17, 6, 58][(i // 16) % 3]
            l4 = {17: P.udp(3, 4, pl), 6: P.tcp(3, 4, pl), 58: P.icmp_echo(128, pl)}[nh]
            r, v6 = P.ipv6(s6, d6, 0, P.hbh(nh, units, rng) + l4), True
        elif t == 10:  # truncated / malformed
            b = bytearray(P.ipv4(s4, d4, 17, P.udp(1, 2, pl)))
            m = (i // 16) % 4
            if m == 0:
                b = b[: int(rng.integers(0, 48))]
            elif m == 1:
                b[4 + 20] ^= 0xFF  # (UDP length lies)
                b[24], b[25] = 0xFF, 0xFF
            elif m == 2:
                b[0] = 0x30 | (b[0] & 15)  # no IP version
            else:
                b[2], b[3] = 0xFF, 0xFF  # total length past the buffer
            r = bytes(b)
        elif t == 11:  # a protocol smoltcp does not checksum / another next header
            r = P.ipv4(s4, d4, 47, pl) if i % 32 < 16 else P.ipv6(s6, d6, 59, pl)
            v6 = i % 32 >= 16
        elif t == 12:  # IPv4 fragments: header only
            r = P.ipv4(s4, d4, 17, P.udp(1, 2, pl), flags_frag=[0x2000, 0x0001, 0x2005][(i // 16) % 3])
        elif t == 13:
            r = P.rand_bytes(rng, int(rng.integers(0, 200)))  # garbage
        elif t == 14:
            r, v6 = P.ipv6(s6, d6, 0, P.hbh(17, i % 4, rng) + P.udp(3, 4, pl)), True  # a short Hop-by-Hop header
        else:
            r = P.ipv4(s4, d4, 6, P.tcp(7, 9, pl))
        if i % 2:
            if t == 13 and i % 4 == 1:
                r, kind = P.eth(r, 0x0806), E.KIND_ETH  # a non-IP ethertype
            else:
                r, kind = P.eth(r, 0x86DD if v6 else 0x0800), E.KIND_ETH
        else:
            kind = E.KIND_IP
        recs.append(r)
        kinds.append(kind)
        flags.append(E.REC_IPHDR_ONLY if i % 5 == 0 else 0)
    return recs, np.array(kinds, dtype=np.uint8), np.array(flags, dtype=np.uint8)


@pytest.fixture(scope="module")
def mixed():
    """~3000 mixed records, packed with random 0-7-byte gaps (odd starts), descriptors shuffled; the
    oracle's emit of them under the default caps."""
    rng = np.random.default_rng(0xFE1D)
    recs, kinds, flags = _mixed_records(rng, 3001)
    host, offs, lens = P.pack(recs, gap_rng=np.random.default_rng(5))
    order = np.random.default_rng(6).permutation(len(recs))
    desc = E.make_descriptors(offs[order], lens[order], kinds[order], flags[order])
    assert int(lens.max()) > 8500 and int(lens.min()) < 64
    return host, desc, Ref(host, desc, len(desc), 0, 0, E.KIND_IP, CAPS_DEFAULT)


def test_descriptor_batch_every_form(eng, mixed):
    host, desc, ref = mixed
    whole, view = _guarded(host)
    dt = torch.from_numpy(desc.view(np.uint8).copy()).to("cuda:0")
    batch = E.Batch(n=len(desc), desc=dt)
    for forced, want in ((AUTO, KERNEL[DWALK]), (DWALK, KERNEL[DWALK]), (WALK, KERNEL[WALK]), (XWALK, KERNEL[WALK])):
        fields = _check(eng, whole, view, batch, ref, CAPS_DEFAULT, forced, want, tag="desc")
    # what the batch holds: a third field, UDP's 0 -> 0xffff, a field past the LDS window, header-only records
    off, val, st = fields["off"], fields["val"], fields["status"]
    assert (off[:, 2] != _lib.NO_FIELD).sum() > 100
    assert ((off[:, 1] != _lib.NO_FIELD) & (val[:, 1] == 0xFFFF)).sum() > 50
    assert (off[:, 1].astype(np.int64) * (off[:, 1] != _lib.NO_FIELD) > 256 + 40).sum() > 50
    assert int(off[:, 1][off[:, 1] != _lib.NO_FIELD].max()) > 2048
    hdr_only = (desc["flags"] & E.REC_IPHDR_ONLY) != 0
    assert (off[hdr_only, 1] == _lib.NO_FIELD).all() and (off[hdr_only, 0] != _lib.NO_FIELD).sum() > 100
    assert (st & E.ST_MALFORMED != 0).sum() > 50 and (st & E.ST_UNSUPPORTED != 0).sum() > 200
    assert ((off == _lib.NO_FIELD).all(axis=1)).sum() > 50  # records with nothing to write


def test_descriptor_batch_in_order_and_tiny(eng, mixed):
    """Descriptors in memory order (back-to-back neighbours in one wavefront), and n = 1 / 7 / 9."""
    host, desc, _ = mixed
    order = np.argsort(desc["offset"])
    whole, view = _guarded(host)
    for n in (1, 7, 9, 1500):
        d = np.ascontiguousarray(desc[order][:n])
        ref = Ref(host, d, n, 0, 0, E.KIND_IP, CAPS_DEFAULT)
        dt = torch.from_numpy(d.view(np.uint8).copy()).to("cuda:0")
        batch = E.Batch(n=n, desc=dt, flags=E.BATCH_FIELD_STORES if n == 7 else 0)  # the flag: accepted, no meaning
        for forced, want in ((AUTO, KERNEL[DWALK]), (WALK, KERNEL[WALK])):
            _check(eng, whole, view, batch, ref, CAPS_DEFAULT, forced, want, tag=("desc-order", n))


# ---------------------------------------------------------------------------------------------
# Caps, launch splitting, streams
# ---------------------------------------------------------------------------------------------


def test_caps(eng):
    """Every cap in {Both, Rx, Tx, None}, one protocol at a time, and all-None, on 64 mixed records."""
    rng = np.random.default_rng(31)
    recs, kinds, flags = _mixed_records(rng, 64)
    host, offs, lens = P.pack(recs, gap_rng=np.random.default_rng(32))
    desc = E.make_descriptors(offs, lens, kinds, flags)
    whole, view = _guarded(host)
    dt = torch.from_numpy(desc.view(np.uint8).copy()).to("cuda:0")
    batch = E.Batch(n=len(desc), desc=dt)
    combos = [tuple(c if j == i else 0 for j in range(5)) for i in range(5) for c in range(4)] + [(3,) * 5]
    for caps in combos:
        ref = Ref(host, desc, len(desc), 0, 0, E.KIND_IP, caps)
        for forced, want in ((AUTO, KERNEL[DWALK]), (WALK, KERNEL[WALK])):
            _check(eng, whole, view, batch, ref, caps, forced, want, tag=("caps", caps))
    # the same records at a fixed stride (padded to one length): the transposed form under every cap
    L = 1600
    fixed = [r[:L] + bytes(L - len(r[:L])) for r in recs]
    fhost = np.frombuffer(b"".join(fixed) + bytes(16), dtype=np.uint8).copy()
    fwhole, fview = _guarded(fhost)
    fb = E.Batch.fixed(len(fixed), L, L, E.KIND_IP)
    for caps in combos:
        ref = Ref(fhost, None, len(fixed), L, L, E.KIND_IP, caps)
        for forced, want in ((AUTO, KERNEL[XWALK]), (WALK, KERNEL[WALK])):
            _check(eng, fwhole, fview, fb, ref, caps, forced, want, tag=("caps-fixed", caps))


def test_launch_records(eng, mixed):
    """set_launch_records(100): the entries advance with the chunks (fixed stride and descriptors)."""
    n, L = 1021, 1500
    t = torch.zeros(n * L + 16, dtype=torch.uint8, device="cuda:0")
    batch = E.Batch.fixed(n, L, L, E.KIND_IP)
    eng.synth(t, batch, E.SYNTH_UDP4, seed=99)
    host = t.cpu().numpy()
    whole, view = _guarded(host)
    ref = Ref(host, None, n, L, L, E.KIND_IP, CAPS_DEFAULT)
    mhost, mdesc, _ = mixed
    mdesc = np.ascontiguousarray(mdesc[:n])
    mref = Ref(mhost, mdesc, n, 0, 0, E.KIND_IP, CAPS_DEFAULT)
    mwhole, mview = _guarded(mhost)
    mbatch = E.Batch(n=n, desc=torch.from_numpy(mdesc.view(np.uint8).copy()).to("cuda:0"))
    eng.set_launch_records(100)
    try:
        for forced, want in ((AUTO, KERNEL[XWALK]), (WALK, KERNEL[WALK])):
            _check(eng, whole, view, batch, ref, CAPS_DEFAULT, forced, want, tag="split")
        for forced, want in ((AUTO, KERNEL[DWALK]), (WALK, KERNEL[WALK])):
            _check(eng, mwhole, mview, mbatch, mref, CAPS_DEFAULT, forced, want, tag="split-desc")
    finally:
        eng.set_launch_records(0)


def test_two_streams_one_context(eng, mixed):
    """Two different buffers on two streams through one context, no synchronisation between the calls."""
    n, L = 1021, 1500
    t = torch.zeros(n * L + 16, dtype=torch.uint8, device="cuda:0")
    batch = E.Batch.fixed(n, L, L, E.KIND_IP)
    eng.synth(t, batch, E.SYNTH_V6MIX, seed=123)
    host = t.cpu().numpy()
    whole, view = _guarded(host)
    ref = Ref(host, None, n, L, L, E.KIND_IP, CAPS_DEFAULT)
    mhost, mdesc, mref = mixed
    mwhole, mview = _guarded(mhost)
    mbatch = E.Batch(n=len(mdesc), desc=torch.from_numpy(mdesc.view(np.uint8).copy()).to("cuda:0"))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for forced, k1, k2 in ((AUTO, KERNEL[XWALK], KERNEL[DWALK]), (WALK, KERNEL[WALK], KERNEL[WALK])):
        before, ent = _prepare(whole, n)
        mbefore, ment = _prepare(mwhole, mref.n)
        torch.cuda.synchronize()  # the buffers are ready; nothing orders the two calls below
        _launch(eng, view, batch, CAPS_DEFAULT, forced, k1, ent, stream=s1, tag="s1")
        _launch(eng, mview, mbatch, CAPS_DEFAULT, forced, k2, ment, stream=s2, tag="s2")
        torch.cuda.synchronize()
        _compare(whole, before, ent, ref, "s1", forced)
        _compare(mwhole, mbefore, ment, mref, "s2", forced)
