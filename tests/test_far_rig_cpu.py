"""The sparse-arena rig of tests/far.py, exercised on the host: seam 2^20, numpy arenas, the oracle's
batch_verify / batch_emit / batch_data standing in for the engine on the sparse layout.

For each placement and for the packed run across the seam: the rig's translated expectations equal the oracle
run directly on the sparse buffer, and Arena.check passes.  Then the faults the rig exists for: a stand-in
that drops the high word of every byte address, and one that stores one stray byte at far_lo - seam, must
fail the comparison or Arena.check, for emit, verify and data, on the STRADDLE and the FAR placement each.
The builders' condition (at least half of the STRADDLE and of the FAR objects accepted by the reference) is
asserted here with the small seam, before any GPU sees the builders."""
import numpy as np
import pytest

from smoltcp_amd import engine as E
from tests import far as F
from tests import pktgen as P

SEAM = 1 << 20
SIZE = SEAM + (1 << 19)
CAPS = [F.NOCAPS, (2, 3, 0, 1, 0)]
PLACEMENTS = {"near": (F.NEAR,), "straddle": (F.NEAR, F.STRADDLE), "far": (F.NEAR, F.FAR_LO, F.FAR_HI),
              "all": (F.NEAR, F.STRADDLE, F.FAR_LO, F.FAR_HI)}


def _records(seed, n=96):
    """Mixed valid-to-be records (the GPU module adds test_gpu_parity's; these need no torch), a few long ones
    and a few of 0-40 random bytes."""
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(n):
        pl = P.rand_bytes(rng, int(rng.integers(0, 300)))
        s4, d4, s6, d6 = P.rand_bytes(rng, 4), P.rand_bytes(rng, 4), P.rand_bytes(rng, 16), P.rand_bytes(rng, 16)
        recs.append([P.ipv4(s4, d4, 17, P.udp(7, 9, pl)), P.ipv4(s4, d4, 6, P.tcp(7, 9, pl)),
                     P.ipv6(s6, d6, 17, P.udp(7, 9, pl)), P.ipv6(s6, d6, 58, P.icmp_echo(128, pl)),
                     P.ipv4(s4, d4, 1, P.icmp_echo(8, pl))][i % 5])
    for i in range(0, n, 19):
        recs[i] = P.ipv4(bytes(4), bytes([1] * 4), 6, P.tcp(1, 2, P.rand_bytes(rng, int(rng.integers(2000, 6000)))))
    for i in range(7, n, 23):
        recs[i] = P.rand_bytes(rng, int(rng.integers(0, 40)))
    return recs


def _case(name, kind=E.KIND_IP):
    recs = _records(len(name))
    if kind == E.KIND_ETH:
        recs = [F.eth_frame(r) for r in recs]
    if name == "run":
        run = F.tcp_run(np.random.default_rng(6), 72, 64, 3000)
        return F.desc_case(SEAM, SIZE, recs, kind, 5, PLACEMENTS["far"], flip_every=5,
                           run=[F.eth_frame(r) for r in run] if kind == E.KIND_ETH else run)
    return F.desc_case(SEAM, SIZE, recs, kind, 5, PLACEMENTS[name], flip_every=5, straddle_below=21 + len(name))


def _arena():
    return F.Arena(SIZE, SEAM, "numpy", slice_bytes=1 << 16)  # several slices, as on the device


def _run(case, op, engine, caps=F.NOCAPS):
    """One call of `engine` on the sparse layout, compared the way the GPU module compares."""
    arena = _arena()
    if op == "emit":
        case.fill(arena, case.raw)
        want, after = case.ref_emit(caps)
    else:
        case.fill(arena)
        want, after = (case.ref_verify(caps) if op == "verify" else case.ref_data()), case.compact
    got = engine(arena, case.desc_far, op, caps)
    assert np.array_equal(got, want), f"{op}: answers differ at {np.flatnonzero(got != want)[:8]}"
    arena.check(case.place.expected(after))


@pytest.mark.parametrize("kind", [E.KIND_IP, E.KIND_ETH])
@pytest.mark.parametrize("name", ["near", "straddle", "far", "all", "run"])
def test_translated_expectations_equal_the_oracle_on_the_sparse_buffer(name, kind):
    case = _case(name, kind)
    st = case.ref_verify()
    F.accepted_enough(case.where, (st & E.ST_ACCEPT) != 0, "verify")
    assert ((st & E.ST_ACCEPT) == 0).any()
    _, after = case.ref_emit()
    changed = np.array([not np.array_equal(after[int(o):int(o + n)], case.raw[int(o):int(o + n)])
                        for o, n in zip(case.offs, case.lens)])
    F.accepted_enough(case.where, changed, "emit")
    want = {"near": {F.NEAR}, "straddle": {F.NEAR, F.STRADDLE}, "far": {F.NEAR, F.FAR_LO, F.FAR_HI},
            "all": {F.NEAR, F.STRADDLE, F.FAR_LO, F.FAR_HI}, "run": {F.NEAR, F.STRADDLE, F.FAR_LO, F.FAR_HI}}[name]
    assert set(case.where.tolist()) == want
    if want > {F.NEAR}:  # one wavefront's 8 descriptors hold near and far records
        w8 = case.where[:case.n // 8 * 8].reshape(-1, 8)
        assert ((w8 == F.NEAR).any(axis=1) & (w8 != F.NEAR).any(axis=1)).sum() >= 1
    for caps in CAPS:
        for op in ("verify", "emit"):
            _run(case, op, F.standin, caps)


def test_data_spans_around_the_seam():
    case = F.data_case(SEAM, SIZE, 9)
    far = case.desc_far
    starts = {int(o) - SEAM for o in far["offset"]}
    ends = {int(o) + int(n) - SEAM for o, n in zip(far["offset"], far["len"])}
    assert set(range(-8, 8)) <= starts and set(range(-8, 8)) <= ends
    for o, n in zip(case.offs, case.lens):  # never the fill throughout
        assert (case.compact[int(o):int(o + n)] != F.DST_FILL).any()
    assert {F.NEAR, F.STRADDLE, F.FAR_LO} <= set(case.where.tolist())
    _run(case, "data", F.standin)


def test_fixed_stride_layout():
    """Records at a sparse fixed stride: one straddles the seam, at least 8 start above it, r * stride
    passes the seam; the oracle on the sparse buffer (stride, base) equals the compact reference."""
    import oracle

    stride, L = (SEAM >> 8) + 37, 97
    fc = F.FixedCase(SEAM, SIZE, stride, L)
    rng = np.random.default_rng(3)
    compact = np.concatenate([np.frombuffer(r, np.uint8) for r in F.tcp_run(rng, fc.n, L, L + 1)])
    assert int(fc.far[-1]) - fc.base > SEAM and fc.base >= 0 and int(fc.far[-1]) + L <= SIZE - F.TAIL
    arena = _arena()
    fc.fill(arena, compact)
    ref = compact.copy()
    st = oracle.batch_emit(ref, None, fc.n, L, L, E.KIND_IP)
    got = oracle.batch_emit(arena.buf[fc.base:], None, fc.n, stride, L, E.KIND_IP)
    assert np.array_equal(got, st)
    arena.check(fc.place.expected(ref))
    vst = oracle.batch_verify(ref, None, fc.n, L, L, E.KIND_IP)
    F.accepted_enough(fc.where, (vst & E.ST_ACCEPT) != 0, "fixed")


@pytest.mark.parametrize("op", ["emit", "verify", "data"])
@pytest.mark.parametrize("name", ["straddle", "far", "run"])
def test_a_dropped_high_word_is_detected(name, op):
    case = F.data_case(SEAM, SIZE, 9) if op == "data" else _case(name)
    if op == "data":  # the data case's spans of one placement, with the NEAR control
        keep = np.isin(case.where, (F.NEAR, F.STRADDLE) if name != "far" else (F.NEAR, F.FAR_LO))
        case = F.DescCase(case.compact, case.offs[keep], case.lens[keep], E.KIND_RAW, case.where[keep], case.place)
    _run(case, op, F.standin)
    with pytest.raises(AssertionError, match="differ|outside every expected extent"):
        _run(case, op, F.standin_dropped_high_word)


def test_a_dropped_high_word_leaves_the_control_alone():
    """The NEAR placement is the control: the faulty stand-in passes it."""
    for op in ("emit", "verify"):
        _run(_case("near"), op, F.standin_dropped_high_word)


@pytest.mark.parametrize("op", ["emit", "verify", "data"])
@pytest.mark.parametrize("name", ["far", "all", "run"])
def test_a_stray_store_below_the_seam_is_detected(name, op):
    case = F.data_case(SEAM, SIZE, 9) if op == "data" else _case(name)
    with pytest.raises(AssertionError, match="outside every expected extent"):
        _run(case, op, F.standin_stray_store)


def test_arena_check_sees_a_byte_next_to_an_extent_and_a_missing_one():
    arena = _arena()
    data = np.arange(100, dtype=np.uint8)
    arena.put(SEAM - 50, data)
    arena.check([(SEAM - 50, data)])
    arena.buf[SEAM + 50] = 0  # inside the margin
    with pytest.raises(AssertionError, match="differ"):
        arena.check([(SEAM - 50, data)])
    arena.refill()
    arena.put(SEAM - 50, data)
    arena.buf[SIZE - 1] = 0  # the arena's last byte
    with pytest.raises(AssertionError, match="outside every expected extent"):
        arena.check([(SEAM - 50, data)])
    arena.refill()
    with pytest.raises(AssertionError, match="differ"):  # an extent that was never written
        arena.check([(SEAM - 50, data)])
    arena.check([])


@pytest.mark.parametrize("seam_at", ["inside", "end", "start", 700])
def test_slot_chain_across_the_seam(seam_at):
    """The destinations of the calls with a second buffer: slots back to back, a third NEAR, a third FAR, a third
    one chain across the seam with the pivot slot at it; the compact form's placement map carries a
    reference's compact arena to the same bytes a run on the sparse arena writes."""
    rng = np.random.default_rng(11)
    caps = rng.integers(0, 1500, 90)
    caps[5], caps[9] = 1460, 0
    compact, far, where, place, total = F.chain_slots_compact(SEAM, SIZE, caps, 5, seam_at, np.random.default_rng(12))
    inside = {"inside": 730, "end": 1460, "start": 0}.get(seam_at, seam_at)
    assert int(far[5]) + inside == SEAM
    assert where[5] == (F.STRADDLE if 0 < inside < 1460 else F.NEAR if inside else F.FAR_LO)
    assert {F.NEAR, F.FAR_LO, F.FAR_HI} <= set(where.tolist())
    order = np.argsort(far.astype(np.int64), kind="stable")
    f, c = far.astype(np.int64)[order], caps[order]
    assert (f[1:] >= f[:-1] + c[:-1]).all(), "slots overlap"
    # a stand-in that writes slot i's bytes at its compact offset and one that writes them at its arena offset
    ref = np.full(total, F.DST_FILL, np.uint8)
    arena = _arena()
    for i in range(len(caps)):
        data = np.full(caps[i], i + 1, np.uint8)
        ref[int(compact[i]):int(compact[i]) + caps[i]] = data
        arena.put(int(far[i]), data)
    arena.check(place.expected(ref))
    arena.buf[int(far[5]) - SEAM + (SEAM if int(far[5]) < SEAM else 0) - 300] ^= 1  # a stray byte 300 below the pivot
    with pytest.raises(AssertionError):
        arena.check(place.expected(ref))


def test_shared_layout_keeps_two_object_sets_apart():
    """A source chain and a descriptor batch in one arena (tcp_segment_emit's templates and payload sources)."""
    rng = np.random.default_rng(13)
    lay = F.Layout(SEAM, SIZE, rng)
    lens = rng.integers(1, 3000, 60)
    _, s_far, swhere, splace, total = F.chain_slots_compact(SEAM, SIZE, lens, 7, "inside", rng, lay)
    case = F.desc_case(SEAM, SIZE, _records(3, 48), E.KIND_IP, 14, (F.NEAR, F.FAR_LO, F.FAR_HI), lay=lay)
    src = rng.integers(0, 256, total, dtype=np.uint8)
    arena = _arena()
    case.fill(arena)
    splace.upload(arena, src)
    arena.check(case.place.expected(case.compact) + splace.expected(src))
    assert swhere[7] == F.STRADDLE and F.STRADDLE not in case.where


# ---- the case builders of the calls with a second buffer, at the small seam ---------------------------------
# Each builder asserts the rig's condition (at least half of the STRADDLE and of the FAR objects accepted,
# delivered, written, cut or answered by the reference) and its placement pairs itself; here they run before
# any GPU sees them, and the sparse layout they return is replayed on a host arena.

BASE = {(a, b) for a in (F.NEAR, F.FAR_LO) for b in (F.NEAR, F.FAR_LO)}


def _replay(case, compact, extents):
    """The records of `compact` and nothing else lie in the first arena; `extents` fit a second one."""
    arena = _arena()
    case.fill(arena, compact)
    arena.check(case.place.expected(compact))
    assert {F.NEAR, F.FAR_LO} <= set(np.where(case.where == F.FAR_HI, F.FAR_LO, case.where).tolist())
    second = _arena()
    for lo, b in extents:
        second.put(lo, b)
    second.check(extents)


@pytest.mark.parametrize("seam_at", ["inside", "end", "start"])
@pytest.mark.parametrize("kind", [E.KIND_IP, E.KIND_ETH])
def test_verify_copy_builder(kind, seam_at):
    c = F.vcopy_case(SEAM, SIZE, kind, seam_at, n=96, long=(2000, 6000))
    assert BASE <= c.pairs and any(a == F.STRADDLE for a, _ in c.pairs)
    at = {int(o) + int(n) for o, n in zip(c.slots["dst_offset"], c.slots["cap"])} | {int(o) for o in c.slots["dst_offset"]}
    assert SEAM in at or seam_at == "inside"
    _replay(c.case, c.case.compact, c.expected)


@pytest.mark.parametrize("seam_at", ["inside", "end"])
def test_copy_emit_builder(seam_at):
    c = F.copy_emit_case(SEAM, SIZE, seam_at)
    assert BASE <= c.pairs and set(c.copies["len"].tolist()) == {0, 1, 15, 16, 17, 1460}
    _replay(c.case, c.after, c.splace.expected(c.src))


@pytest.mark.parametrize("rot", [0, 1, 2])
def test_tcp_assemble_builder(rot):
    c = F.tcpasm_case(SEAM, SIZE, rot)
    lo, rl = int(c.wins["dst_offset"][c.ring_of.index(0)]), int(c.wins["ring_len"][0])
    assert lo < SEAM < lo + rl and (F.STRADDLE, (F.STRADDLE, F.NEAR, F.FAR_LO)[c.ring_of[0]]) in c.pairs
    _replay(c.case, c.case.compact, c.dplace.expected(c.ref_arena))


@pytest.mark.parametrize("seam_at", ["inside", "end", "far-inside"])
@pytest.mark.parametrize("kind", [E.KIND_IP, E.KIND_ETH])
def test_echo_reply_builder(kind, seam_at):
    c = F.echo_case(SEAM, SIZE, kind, seam_at)
    assert BASE <= c.pairs
    _replay(c.case, c.case.compact, c.dplace.expected(c.ref_arena))


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("seam_at", sorted(F.SEAM_IN_RUN))
def test_cut_builders(seam_at, strided):
    """fragment_emit and tcp_segment_emit: the seam lies between two frames of a run or inside a frame."""
    c = F.fragcut_case(SEAM, SIZE, seam_at, strided)
    assert BASE <= c.pairs and (c.dwhere == F.STRADDLE).sum() == 1
    i = int(np.flatnonzero(c.dwhere == F.STRADDLE)[0])
    S = c.stride or int(c.ref_out["frame_len"][i])
    assert (SEAM - int(c.plans["dst_offset"][i])) % S == (0 if seam_at == "between" else int(c.ref_out["frame_len"][i]) // 2)
    _replay(c.case, c.case.raw, c.dplace.expected(c.ref_arena))
    t = F.tcpcut_case(SEAM, SIZE, seam_at, strided)
    so, ln = int(t.plans["src_offset"][7]), int(t.plans["len"][7])
    assert BASE <= t.pairs and so < SEAM < so + ln  # a send's payload source crosses the seam
    arena = _arena()
    t.case.fill(arena, t.case.raw)
    t.splace.upload(arena, t.src)
    arena.check(t.case.place.expected(t.case.raw) + t.splace.expected(t.src))


@pytest.mark.parametrize("seam_at", ["inside", "end"])
def test_fragment_groups_builder(seam_at):
    """The drop-in route: the builder asserts that the oracle's group emit over the offloaded fragments equals
    tx_pair's emit-whole-then-fragment reference and that verify_frag accepts all of it."""
    c = F.fraggroups_case(SEAM, SIZE, seam_at)
    assert (c.ref_st & E.ST_ACCEPT).all() and not np.array_equal(c.emitted, c.case.raw)
    _replay(c.case, c.emitted, c.dplace.expected(c.ref_arena))


def test_nhc_builder(golden):
    k = golden["sixlowpan_nhc_udp"][0]
    c = F.nhc_case(SEAM, SIZE, bytes.fromhex(k["bytes"]), bytes.fromhex(k["src"]) + bytes.fromhex(k["dst"]))
    _replay(c.case, c.after, [])
