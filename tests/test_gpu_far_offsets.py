"""Every batched call with 64-bit byte offsets at and past 4 GiB, on the sparse-arena rig of tests/far.py.

The arenas hold 2^32 + 2^28 bytes of the sentinel; records, payload sources, slots, rings and frame runs lie
wholly below 2^32 (NEAR, the control), across it (STRADDLE) and wholly above it (FAR, low words small and
large).  Cases are built compactly, the references (the oracle, tests/*_ref.py) run on the compact buffers,
and the placement map moves every object into the arena and rewrites the offsets.  Everything is compared
exactly: status bytes and entries as they are, the arena through Arena.check (every expected extent with 256
bytes around it on the host, every other byte against the sentinel on the device), so a store whose high
word was dropped shows at its offset mod 2^32 and a load whose high word was dropped reads the sentinel
(each test asserts first that the reference accepts at least half of the STRADDLE and of the FAR objects).

The module skips only when the device has less than 12 GiB free."""
import ctypes

import numpy as np
import pytest

import oracle
from tests import far as F
from tests import pktgen as P

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from smoltcp_amd import _lib  # noqa: E402
from smoltcp_amd import engine as E  # noqa: E402
from tests.engines import VariantEngine  # noqa: E402
from tests.test_gpu_parity import FIXED_STRIDE_VARIANTS, WIDE_KERNELS, _expected_launch, _kv, _mixed_records  # noqa: E402

SEAM, SIZE = F.GPU_SEAM, F.GPU_SIZE
CAPS = [F.NOCAPS, (2, 3, 0, 1, 0)]
F_XWALK, V_NOSTORE = 2, 32
NUMBERS, PER_GROUP = 128, 16  # the registry's number space (csum_variants.h), swept in groups: one test each
GROUPS = NUMBERS // PER_GROUP
F_WALK, F_TILE, F_DWALK = 0, 1, 3


class Rig:
    def __init__(self):
        self.eng = VariantEngine(0)
        self.a = F.Arena(SIZE, SEAM, "torch")
        self._b = None
        L, info = _lib.lib(), (ctypes.c_int * 4)()
        rows = [v for v in range(NUMBERS) if L.smol_csum_tool_variant_info(v, info) == 0 and not info[1] & V_NOSTORE]
        self.variants = [-1] + self.eng.avail(rows)
        self.family = {}
        for v in rows:
            L.smol_csum_tool_variant_info(v, info)
            self.family[v] = info[0]
        self.cache = {}

    @property
    def b(self):
        """The second buffer's arena, made when a call with a second buffer first needs it."""
        if self._b is None:
            self._b = F.Arena(SIZE, SEAM, "torch")
        return self._b

    def group(self, g):
        return [v for v in self.variants if v // PER_GROUP == g or (v == -1 and g == 0)]

    def close(self):
        self.eng.close()
        self.a.buf = None
        if self._b is not None:
            self._b.buf = None
        self.cache.clear()
        torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def rig():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    free, _ = torch.cuda.mem_get_info(0)
    if free < 12 << 30:
        pytest.skip(f"needs 12 GiB of free device memory, {free / 2**30:.1f} GiB free")
    r = Rig()
    yield r
    r.close()
    del r


def _dev(a: np.ndarray):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _pre(*shape):
    return torch.full(shape, F.PRE_FILL, dtype=torch.uint8, device="cuda")


def test_the_registry_sweep_is_whole(rig):
    """Every family is in the sweep: the walk kernel, the tile kernel, the transposed walk, the descriptor
    walk (staged forms with their segment passes included), and all groups together hold every row."""
    L, info = _lib.lib(), (ctypes.c_int * 4)()
    assert L.smol_csum_tool_variant_info(NUMBERS, info) != 0, "the registry has numbers past the sweep"
    assert {F_WALK, F_TILE, F_XWALK, F_DWALK} <= {rig.family[v] for v in rig.variants if v >= 0}
    assert sorted(v for g in range(GROUPS) for v in rig.group(g)) == sorted(rig.variants)


# ---- verify / emit / data over descriptor batches ----------------------------------------------------------

def _desc_records(kind, seed=56):
    """test_gpu_parity's mixed records, records of 20-60 KB and records of 0-40 B."""
    rng = np.random.default_rng(seed)
    recs = _mixed_records(rng, 400)
    for i in range(0, 400, 37):
        recs[i] = P.ipv4(bytes([192, 168, 1, 1]), bytes([192, 168, 1, 2]), 6,
                         P.tcp(1, 2, P.rand_bytes(rng, int(rng.integers(20000, 60000)))))
    for i in range(5, 400, 41):
        recs[i] = P.rand_bytes(rng, int(rng.integers(0, 40)))
    return [F.eth_frame(r) for r in recs] if kind == E.KIND_ETH else recs


def _desc_case(rig, kind, which):
    """(case, per caps: verify statuses, emit statuses, the compact buffer after emit), built and answered by
    the oracle once, shared by the variants.  which: "record" (one record straddles 2^32: a 20-60 KB one cut
    in its payload for IP, a short one cut in its IP header for Ethernet) or "run" (the packed run does)."""
    key = ("desc", kind, which)
    if key not in rig.cache:
        recs = _desc_records(kind)
        if which == "run":
            run = F.tcp_run(np.random.default_rng(72), 72, 64, 9001)
            case = F.desc_case(SEAM, SIZE, recs, kind, 7, (F.NEAR, F.FAR_LO, F.FAR_HI), flip_every=5,
                               run=[F.eth_frame(r) for r in run] if kind == E.KIND_ETH else run)
        elif kind == E.KIND_IP:
            case = F.desc_case(SEAM, SIZE, recs, kind, 8, flip_every=5, straddle_index=37, straddle_below=8000)
        else:
            case = F.desc_case(SEAM, SIZE, recs, kind, 9, flip_every=5, straddle_below=21)
        assert {F.NEAR, F.STRADDLE, F.FAR_LO, F.FAR_HI} <= set(case.where.tolist())
        refs = {}
        for caps in CAPS:
            st = case.ref_verify(caps)
            est, after = case.ref_emit(caps)
            refs[caps] = (st, est, after)
        st, _, after = refs[F.NOCAPS]
        F.accepted_enough(case.where, (st & E.ST_ACCEPT) != 0, "verify")
        changed = [not np.array_equal(after[int(o):int(o + n)], case.raw[int(o):int(o + n)])
                   for o, n in zip(case.offs, case.lens)]
        F.accepted_enough(case.where, changed, "emit")
        case.batch = E.Batch(n=case.n, desc=_dev(case.desc_far))
        rig.cache[key] = (case, refs)
    return rig.cache[key]


def _assert_desc_launch(v, op, launched, want_kernel):
    assert launched["kernel"] == want_kernel, (v, op, launched, want_kernel)
    if op == "verify" and v in (56, 60, 63, 41):  # as test_gpu_parity._run_records asserts them
        assert _kv(launched) == ("dwalk_kernel", 63 if v == 41 else v), (v, launched)
    if op == "emit" and v in (61, 62, 63, 18, 20, 41, 94):
        assert _kv(launched) == ("dwalk_kernel", v), (v, launched)


@pytest.mark.parametrize("group", range(GROUPS))
@pytest.mark.parametrize("caps", CAPS, ids=["default", "caps23010"])
@pytest.mark.parametrize("which", ["record", "run"])
@pytest.mark.parametrize("kind", [E.KIND_IP, E.KIND_ETH])
def test_descriptor_batches_verify_and_emit(rig, kind, which, caps, group):
    """Shuffled NEAR / STRADDLE / FAR descriptors (each wavefront of the descriptor walk holds near and far
    records) and, for "run", 72 packed in-order records of 64-9000 B across 2^32, the carry inside one
    wavefront's 8 records: default dispatch and every storing variant of the registry, forced; default caps
    and (2, 3, 0, 1, 0).  The arena is checked after every emit and once after the verifies."""
    eng, arena = rig.eng, rig.a
    case, refs = _desc_case(rig, kind, which)
    variants = rig.group(group)
    launched = set()
    case.fill(arena)
    for v in variants:
        eng.set_variant(v)
        try:
            want_k = eng.kernel_for("verify", case.batch)
            st = eng.verify(arena.buf, case.batch, caps=caps, status=_pre(case.n)).cpu().numpy()
            lv = eng.last_launch()
            _assert_desc_launch(v, "verify", lv, want_k)
            launched.add(("verify",) + _kv(lv))
            bad = np.flatnonzero(st != refs[caps][0])
            assert bad.size == 0, (v, caps, bad[:8], case.where[bad[:8]], st[bad[:8]], refs[caps][0][bad[:8]])
        finally:
            eng.set_variant(-1)
    arena.check(case.place.expected(case.compact))  # verify only reads
    case.fill(arena, case.raw)
    for v in variants:
        eng.set_variant(v)
        try:
            want_k = eng.kernel_for("emit", case.batch)
            est = eng.emit(arena.buf, case.batch, caps=caps, status=_pre(case.n)).cpu().numpy()
            le = eng.last_launch()
        finally:
            eng.set_variant(-1)
        _assert_desc_launch(v, "emit", le, want_k)
        launched.add(("emit",) + _kv(le))
        assert np.array_equal(est, refs[caps][1]), (v, caps, np.flatnonzero(est != refs[caps][1])[:8])
        try:
            arena.check(case.place.expected(refs[caps][2]))
        except AssertionError as e:
            raise AssertionError(f"emit, variant {v}, caps {caps}: {e}") from None
        case.place.upload(arena, case.raw)
    print(f"far descriptor batches kind {kind} {which} group {group}: {sorted(launched)}")


@pytest.mark.parametrize("group", range(GROUPS))
def test_data_spans_across_the_seam(rig, group):
    """data() over raw spans of 1, 2, 63, 64, 1500 and 131075 bytes that begin, and that end, at every byte of
    the 16-byte window around 2^32, random and 0xFF bytes; the same lengths NEAR and FAR."""
    eng, arena = rig.eng, rig.a
    if "data" not in rig.cache:
        case = F.data_case(SEAM, SIZE, 15)
        for o, n in zip(case.offs, case.lens):
            assert (case.compact[int(o):int(o + n)] != F.DST_FILL).any()
        case.batch = E.Batch(n=case.n, desc=_dev(case.desc_far))
        rig.cache["data"] = (case, case.ref_data())
    case, ref = rig.cache["data"]
    assert {F.NEAR, F.STRADDLE, F.FAR_LO} <= set(case.where.tolist())
    case.fill(arena)
    launched = set()
    for v in rig.group(group):
        eng.set_variant(v)
        try:
            want_k = eng.kernel_for("data", case.batch)
            out = eng.data(arena.buf, case.batch).cpu().numpy().view(np.uint16)
            ld = eng.last_launch()
        finally:
            eng.set_variant(-1)
        assert ld["kernel"] == want_k, (v, ld)
        launched.add(_kv(ld))
        bad = np.flatnonzero(out != ref)
        assert bad.size == 0, (v, bad[:8], case.desc_far[bad[:8]], out[bad[:8]], ref[bad[:8]])
    arena.check(case.place.expected(case.compact))
    print(f"far data group {group}: {sorted(launched)}")


# ---- verify / emit at a sparse fixed stride ----------------------------------------------------------------

STRIDE = (1 << 24) + 37
FIXED = {97: E.SYNTH_TCP4, 1500: E.SYNTH_UDP4, 1922: E.SYNTH_TCP4, 3970: E.SYNTH_V6MIX, 8066: E.SYNTH_UDP4}


def _fixed_case(rig, L):
    key = ("fixed", L)
    if key not in rig.cache:
        fc = F.FixedCase(SEAM, SIZE, STRIDE, L)
        assert int((fc.far >= SEAM).sum()) >= 8 and int(fc.far[-1]) - fc.base >= 1 << 32  # r * stride passes 2^32
        tmp = torch.zeros(fc.n * L + 64, dtype=torch.uint8, device="cuda")
        rig.eng.synth(tmp, E.Batch.fixed(fc.n, L, L, E.KIND_IP), FIXED[L], seed=L)
        fc.raw = tmp.cpu().numpy()[:fc.n * L].copy()
        fc.compact = fc.raw.copy()
        oracle.batch_emit(fc.compact, None, fc.n, L, L, E.KIND_IP)
        for i in range(2, fc.n, 7):
            fc.compact[i * L + L // 2] ^= 0x04
        refs = {}
        for caps in CAPS:
            after = fc.raw.copy()
            est = oracle.batch_emit(after, None, fc.n, L, L, E.KIND_IP, caps)
            refs[caps] = (oracle.batch_verify(fc.compact.copy(), None, fc.n, L, L, E.KIND_IP, caps), est, after)
        F.accepted_enough(fc.where, (refs[F.NOCAPS][0] & E.ST_ACCEPT) != 0, "fixed verify")
        F.accepted_enough(fc.where, (refs[F.NOCAPS][2] != fc.raw).reshape(fc.n, L).any(axis=1), "fixed emit")
        fc.batch = E.Batch.fixed(fc.n, STRIDE, L, E.KIND_IP)
        rig.cache[key] = (fc, refs)
    return rig.cache[key]


def _assert_fixed_launch(rig, v, op, launched, want_kernel, L):
    assert launched["kernel"] == want_kernel, (v, op, L, launched, want_kernel)
    if v in FIXED_STRIDE_VARIANTS and rig.family[v] in (F_WALK, F_TILE) and L <= 4000:  # test_variants_fixed_stride's lengths
        assert _kv(launched) == _expected_launch(v, op, False), (v, op, L, launched)
    if launched["kernel"] == "xwalk_kernel" and rig.family.get(v) == F_XWALK:  # as test_gpu_xwalk_variants asserts them
        assert launched["variant"] == v, (v, op, L, launched)
    if v in WIDE_KERNELS and WIDE_KERNELS[v][0] == "xwalk_kernel" and L >= 1024:
        assert launched["kernel"] == "xwalk_kernel", (v, op, L, launched)


@pytest.mark.parametrize("group", range(GROUPS))
@pytest.mark.parametrize("caps", CAPS, ids=["default", "caps23010"])
@pytest.mark.parametrize("L", sorted(FIXED))
def test_sparse_fixed_stride_verify_and_emit(rig, L, caps, group):
    """Batch.fixed(n, 2^24 + 37, L) from a base that makes one record straddle 2^32: about 272 records, 16 of
    them above 2^32, r * stride past 2^32 in every kernel that serves the stride; records synthesized
    compactly on the device and placed; default dispatch and every storing variant, both caps."""
    eng, arena = rig.eng, rig.a
    fc, refs = _fixed_case(rig, L)
    view = arena.buf[fc.base:]
    launched = set()
    fc.fill(arena, fc.compact)
    for v in rig.group(group):
        eng.set_variant(v)
        try:
            want_k = eng.kernel_for("verify", fc.batch)
            st = eng.verify(view, fc.batch, caps=caps, status=_pre(fc.n)).cpu().numpy()
            lv = eng.last_launch()
            _assert_fixed_launch(rig, v, "verify", lv, want_k, L)
            launched.add(("verify",) + _kv(lv))
            bad = np.flatnonzero(st != refs[caps][0])
            assert bad.size == 0, (v, caps, bad[:8], fc.where[bad[:8]], st[bad[:8]], refs[caps][0][bad[:8]])
        finally:
            eng.set_variant(-1)
    arena.check(fc.place.expected(fc.compact))
    fc.fill(arena, fc.raw)
    for v in rig.group(group):
        eng.set_variant(v)
        try:
            want_k = eng.kernel_for("emit", fc.batch)
            est = eng.emit(view, fc.batch, caps=caps, status=_pre(fc.n)).cpu().numpy()
            le = eng.last_launch()
        finally:
            eng.set_variant(-1)
        _assert_fixed_launch(rig, v, "emit", le, want_k, L)
        launched.add(("emit",) + _kv(le))
        assert np.array_equal(est, refs[caps][1]), (v, caps, np.flatnonzero(est != refs[caps][1])[:8])
        try:
            arena.check(fc.place.expected(refs[caps][2]))
        except AssertionError as e:
            raise AssertionError(f"emit, variant {v}, caps {caps}, L {L}: {e}") from None
        fc.place.upload(arena, fc.raw)
    print(f"far fixed stride L {L} group {group}: {sorted(launched)}")


# ---- verify / emit, dense across the seam ------------------------------------------------------------------

def _gather(buf2d, idx):
    return buf2d.index_select(0, idx).cpu().numpy().reshape(-1).copy()


@pytest.mark.parametrize("L", [1500, 9000])
def test_dense_batch_across_the_seam(rig, L):
    """ceil(2^32 / L) + 4099 packed records synthesized on the device: tests/test_gpu_c5.py's three
    properties at a size that runs where C5 skips, lines shared by neighbours on both sides of 2^32.  The
    oracle's sample: the 600 records around record 2^32 // L, the first and the last 64, 4096 drawn uniformly."""
    eng, arena = rig.eng.prod, rig.a
    n = -(-(1 << 32) // L) + 4099
    assert n * L <= SIZE
    arena.refill()
    buf = arena.buf[:n * L]
    batch = E.Batch.fixed(n, L, L, E.KIND_IP)
    eng.synth(buf, batch, E.SYNTH_UDP4, seed=0x5EED0005 + L)
    rng = np.random.default_rng(0xC5 + L)
    mid = (1 << 32) // L
    idx = np.unique(np.concatenate([np.arange(mid - 300, mid + 300), np.arange(64), np.arange(n - 64, n),
                                    rng.choice(n, 4096, replace=False)]))
    ns = idx.size
    idx_t = torch.from_numpy(idx.astype(np.int64)).cuda()
    b2 = buf.view(n, L)
    before = _gather(b2, idx_t)

    want_k = eng.kernel_for("emit", batch)
    eng.emit(buf, batch)
    le = eng.last_launch()
    assert le["kernel"] == want_k, le
    after = _gather(b2, idx_t)
    ref = before.copy()
    oracle.batch_emit(ref, None, ns, L, L, E.KIND_IP, F.NOCAPS)
    bad = np.flatnonzero((after != ref).reshape(ns, L).any(axis=1))
    assert bad.size == 0, f"device emit differs from the oracle on sampled records {idx[bad[:8]]}"

    want_k = eng.kernel_for("verify", batch)
    st = eng.verify(buf, batch)
    lv = eng.last_launch()
    assert lv["kernel"] == want_k, lv
    assert int(((st & E.ST_ACCEPT) != 0).sum()) == n, "an emitted record was rejected"

    eng.corrupt(buf, batch, every=64, seed=0xC5)
    st = eng.verify(buf, batch)
    rejected = (st & E.ST_ACCEPT) == 0
    n64 = n // 64 * 64
    # only corrupted records (every 64th, as corrupt_kernel picks them) are rejected ...
    assert int(rejected[:n64].view(-1, 64)[:, 1:].sum()) == 0 and int(rejected[n64 + 1:].sum()) == 0
    # ... and a corrupted record the device accepts is one the reference accepts too
    first = torch.arange(0, n, 64, device="cuda")
    missed = first[~rejected.index_select(0, first)]
    assert missed.numel() <= 64, f"{missed.numel()} corrupted records accepted"
    if missed.numel():
        m_st = oracle.batch_verify(_gather(b2, missed), None, missed.numel(), L, L, E.KIND_IP, F.NOCAPS)
        assert np.array_equal(st.index_select(0, missed).cpu().numpy(), m_st)
        assert ((m_st & E.ST_ACCEPT) != 0).all()
    corrupted = _gather(b2, idx_t)
    ref_st = oracle.batch_verify(corrupted, None, ns, L, L, E.KIND_IP, F.NOCAPS)
    got_st = st.index_select(0, idx_t).cpu().numpy()
    assert np.array_equal(got_st, ref_st), idx[np.flatnonzero(got_st != ref_st)[:8]]
    assert bool((arena.buf[n * L:] == F.DST_FILL).all()), "a byte past the batch was written"
    print(f"far dense L {L}: emit {_kv(le)}, verify {_kv(lv)}; {n} records, {int(rejected.sum())} rejected of "
          f"{-(-n // 64)} corrupted")


# ---- emit_fields: the values out, the frames patched on the host -------------------------------------------

FK_AUTO, FK_WALK, FK_XWALK, FK_DWALK = 0, 1, 2, 3
FK_KERNEL = {FK_WALK: "csum_fields_kernel", FK_XWALK: "xwalk_kernel(fields)", FK_DWALK: "dwalk_kernel(fields)"}


def _fields_check(rig, view, batch, n, forced, serves, caps, host, offs, lens, want_after, want_st, tag):
    """One emit_fields call: the forced form runs where it serves the batch (else the walk kernel's), the
    entries applied to `host` on the host equal the oracle's emit, the statuses equal emit's, the 8 entries
    past n keep their fill."""
    eng = rig.eng.prod
    ent = _pre(n + 8, 16)
    eng.set_fields_kernel(forced)
    try:
        eng.emit_fields(view, batch, caps=caps, fields=ent)
        launched = eng.last_launch()
    finally:
        eng.set_fields_kernel(FK_AUTO)
    if forced != FK_AUTO:
        assert launched["kernel"] == FK_KERNEL[forced if serves else FK_WALK], (tag, forced, launched)
    e = ent.cpu().numpy()
    assert (e[n:] == F.PRE_FILL).all(), (tag, forced, "entries past n written")
    f = e[:n].reshape(-1).view(E.FIELDS_DTYPE)
    patched = host.copy()
    ok = E.apply_fields(patched, offs, lens, f)
    assert ok.all(), (tag, forced, np.flatnonzero(~ok)[:8])
    bad = np.flatnonzero(f["status"] != want_st)
    assert bad.size == 0, (tag, forced, bad[:8], f["status"][bad[:8]], want_st[bad[:8]])
    diff = np.flatnonzero(patched != want_after)
    assert diff.size == 0, (tag, forced, "patched bytes differ from the oracle's emit at", diff[:8])
    return launched["kernel"]


@pytest.mark.parametrize("which", ["record", "run"])
@pytest.mark.parametrize("kind", [E.KIND_IP, E.KIND_ETH])
def test_emit_fields_descriptor_batches(rig, kind, which):
    """emit_fields over the NEAR / STRADDLE / FAR descriptor batches: the library's choice and the three
    forced forms (the transposed walk gives way to the walk kernel); apply_fields on the compact host copy
    equals the oracle's emit.  The arena is only read."""
    case, refs = _desc_case(rig, kind, which)
    case.fill(rig.a, case.raw)
    ran = set()
    for caps in CAPS:
        for forced in (FK_AUTO, FK_WALK, FK_XWALK, FK_DWALK):
            ran.add(_fields_check(rig, rig.a.buf, case.batch, case.n, forced, forced != FK_XWALK, caps, case.raw,
                                  case.offs.astype(np.int64), case.lens.astype(np.int64), refs[caps][2], refs[caps][1],
                                  (kind, which, caps)))
    rig.a.check(case.place.expected(case.raw))
    print(f"far emit_fields kind {kind} {which}: {sorted(ran)}")


@pytest.mark.parametrize("L", sorted(FIXED))
def test_emit_fields_sparse_fixed_stride(rig, L):
    """emit_fields over the sparse fixed-stride batches (r * stride past 2^32): the library's choice and the
    forced forms (the descriptor walk gives way; the transposed walk serves 1024 B and up)."""
    fc, refs = _fixed_case(rig, L)
    fc.fill(rig.a, fc.raw)
    ran = set()
    for caps in CAPS:
        for forced in (FK_AUTO, FK_WALK, FK_XWALK, FK_DWALK):
            ran.add(_fields_check(rig, rig.a.buf[fc.base:], fc.batch, fc.n, forced, forced == FK_WALK or
                                  (forced == FK_XWALK and L >= 1024), caps, fc.raw, np.arange(fc.n, dtype=np.int64) * L, L,
                                  refs[caps][2], refs[caps][1], (L, caps)))
    rig.a.check(fc.place.expected(fc.raw))
    print(f"far emit_fields fixed L {L}: {sorted(ran)}")


# ---- the calls with a second buffer: tests/far.py builds each case and asserts its conditions ---------------

@pytest.mark.parametrize("seam_at", ["inside", "end", "start"])
@pytest.mark.parametrize("kind", [E.KIND_IP, E.KIND_ETH])
def test_verify_copy_slots_across_the_seam(rig, kind, seam_at):
    """F.vcopy_case; every launch shape.  Status bytes equal verify's oracle, spans
    tests/test_verify_copy_cpu.py's rule, the destination arena is checked whole."""
    eng = rig.eng.prod
    c = F.vcopy_case(SEAM, SIZE, kind, seam_at)
    case, n, slots = c.case, c.case.n, _dev(c.slots)
    case.fill(rig.a)
    for shape in range(9):
        rig.b.refill()
        eng.set_shape(shape)
        try:
            st, sp = eng.verify_copy(rig.a.buf, case.batch_of(), rig.b.buf, slots, status=_pre(n), spans=_pre(n, 8))
            launched = eng.last_launch()
        finally:
            eng.set_shape(-1)
        assert launched["kernel"] == "vcopy_kernel" and launched["variant"] == 0, launched
        got_st, got_sp = st.cpu().numpy(), sp.cpu().numpy().reshape(-1).view(E.SPAN_DTYPE)
        assert np.array_equal(got_st, c.ref_st), (shape, np.flatnonzero(got_st != c.ref_st)[:8])
        bad = np.flatnonzero(got_sp != c.ref_sp)
        assert bad.size == 0, (shape, bad[:8], got_sp[bad[:4]], c.ref_sp[bad[:4]], case.where[bad[:4]], c.dwhere[bad[:4]])
        try:
            rig.b.check(c.expected)
        except AssertionError as e:
            raise AssertionError(f"shape {shape}: {e}") from None
    rig.a.check(case.place.expected(case.compact))
    print(f"far verify_copy kind {kind} {seam_at}: vcopy_kernel, pairs {sorted(c.pairs)}")


@pytest.mark.parametrize("seam_at", ["inside", "end"])
def test_copy_emit_sources_across_the_seam(rig, seam_at):
    """F.copy_emit_case; the library's choice and every forced copy-emit variant of tests/test_gpu_copy_emit.py.
    Records and status bytes equal oracle.batch_copy_emit's on the compact buffers; the sources are only read."""
    from tests.test_gpu_copy_emit import COPY_VARIANTS

    eng = rig.eng
    c = F.copy_emit_case(SEAM, SIZE, seam_at)
    case, n, copies = c.case, c.case.n, _dev(c.copies)
    rig.b.refill()
    c.splace.upload(rig.b, c.src)
    case.fill(rig.a, case.raw)
    ran = set()
    for v in eng.avail(COPY_VARIANTS):
        eng.set_variant(v)
        try:
            st = eng.copy_emit(rig.a.buf, case.batch_of(), rig.b.buf, copies, status=_pre(n))
            launched = eng.last_launch()
        finally:
            eng.set_variant(-1)
        want = ("csum_kernel", v) if v in (1, 8, 11, 16) else ("copy_kernel", v if v in (17, 22, 30, 98, 102) else 21)
        assert _kv(launched) == want, (v, launched)  # as tests/test_gpu_copy_emit.py asserts it
        ran.add(_kv(launched))
        assert np.array_equal(st.cpu().numpy(), c.ref_st), (v, np.flatnonzero(st.cpu().numpy() != c.ref_st)[:8])
        try:
            rig.a.check(case.place.expected(c.after))
        except AssertionError as e:
            raise AssertionError(f"variant {v}: {e}") from None
        case.place.upload(rig.a, case.raw)
    rig.b.check(c.splace.expected(c.src))
    print(f"far copy_emit {seam_at}: {sorted(ran)}")


@pytest.mark.parametrize("rot", [0, 1, 2])
def test_tcp_assemble_rings_across_the_seam(rig, rot):
    """F.tcpasm_case.  Status bytes, segment and flow entries equal tests/tcp_assemble_ref.py's; the rings'
    arena is checked whole."""
    eng = rig.eng.prod
    c = F.tcpasm_case(SEAM, SIZE, rot)
    case, n = c.case, c.case.n
    case.fill(rig.a)
    rig.b.refill()
    st, sg, fl = eng.verify_tcp_assemble(rig.a.buf, case.batch_of(), _dev(c.groups), rig.b.buf, _dev(c.wins), status=_pre(n),
                                         segs=_pre(n, 16))
    launched = eng.last_launch()
    assert launched["kernel"] == "tcpasm_kernel" and launched["G"] == 64, launched
    assert np.array_equal(st.cpu().numpy(), c.ref_st)
    got_sg = sg.cpu().numpy().reshape(-1).view(E.TCPSEG_DTYPE)
    bad = np.flatnonzero(got_sg != c.ref_segs)
    assert bad.size == 0, (bad[:8], got_sg[bad[:4]], c.ref_segs[bad[:4]])
    got_fl = fl.cpu().numpy().reshape(-1).view(E.TCPFLOW_DTYPE)
    assert np.array_equal(got_fl, c.ref_flows), (got_fl, c.ref_flows)
    rig.b.check(c.dplace.expected(c.ref_arena))
    rig.a.check(case.place.expected(case.compact))
    print(f"far verify_tcp_assemble rot {rot}: {launched['kernel']}, rings {c.ring_of}")


@pytest.mark.parametrize("seam_at", ["inside", "end", "far-inside"])
@pytest.mark.parametrize("kind", [E.KIND_IP, E.KIND_ETH])
def test_echo_reply_slots_across_the_seam(rig, kind, seam_at):
    """F.echo_case; every launch shape of the kernel's shape set.  Status bytes, entries and the replies' arena
    equal tests/echo_ref.py's."""
    from tests.test_gpu_echo_reply import SHAPES

    eng = rig.eng.prod
    c = F.echo_case(SEAM, SIZE, kind, seam_at)
    case, n, slots = c.case, c.case.n, _dev(c.slots)
    case.fill(rig.a)
    for shape in sorted(SHAPES):
        rig.b.refill()
        eng.set_shape(shape)
        try:
            st, ent = eng.verify_echo_reply(rig.a.buf, case.batch_of(), rig.b.buf, slots, status=_pre(n), echo=_pre(n, 8))
            launched = eng.last_launch()
        finally:
            eng.set_shape(-1)
        assert launched["kernel"] == "echo" and launched["variant"] == 0, launched
        assert (launched["G"], launched["U"]) == SHAPES[shape], launched
        got_st, got_ent = st.cpu().numpy(), ent.cpu().numpy().reshape(-1).view(E.ECHO_DTYPE)
        assert np.array_equal(got_st, c.ref_st), (shape, np.flatnonzero(got_st != c.ref_st)[:8])
        bad = np.flatnonzero(got_ent != c.ref_ent)
        assert bad.size == 0, (shape, bad[:8], got_ent[bad[:4]], c.ref_ent[bad[:4]], case.where[bad[:4]], c.dwhere[bad[:4]])
        try:
            rig.b.check(c.dplace.expected(c.ref_arena))
        except AssertionError as e:
            raise AssertionError(f"shape {shape}: {e}") from None
    rig.a.check(case.place.expected(case.compact))
    print(f"far verify_echo_reply kind {kind} {seam_at}: echo, shapes {sorted(SHAPES)}")


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("seam_at", sorted(F.SEAM_IN_RUN))
def test_fragment_emit_frame_runs_across_the_seam(rig, seam_at, strided):
    """F.fragcut_case.  Entries and the frames' arena equal tests/fragment_ref.py's; the datagrams are only read."""
    eng = rig.eng.prod
    c = F.fragcut_case(SEAM, SIZE, seam_at, strided)
    case, n = c.case, c.case.n
    case.fill(rig.a, case.raw)
    rig.b.refill()
    out = eng.fragment_emit(rig.a.buf, case.batch_of(), rig.b.buf, _dev(c.plans), frame_stride=c.stride, out=_pre(n, 16))
    launched = eng.last_launch()
    assert launched["kernel"] == "fragcut_kernel", launched
    got = out.cpu().numpy().reshape(-1).view(E.FRAGOUT_DTYPE)
    bad = np.flatnonzero(got != c.ref_out.view(E.FRAGOUT_DTYPE))
    assert bad.size == 0, (bad[:8], got[bad[:4]], c.ref_out[bad[:4]], case.where[bad[:4]], c.dwhere[bad[:4]])
    rig.b.check(c.dplace.expected(c.ref_arena))
    rig.a.check(case.place.expected(case.raw))
    print(f"far fragment_emit {seam_at} stride {c.stride}: {launched['kernel']}")


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("seam_at", sorted(F.SEAM_IN_RUN))
def test_tcp_segment_emit_frame_runs_and_source_across_the_seam(rig, seam_at, strided):
    """F.tcpcut_case.  Entries and the frames' arena equal tests/tcp_segment_ref.py's; templates and sources,
    both in the first arena, are only read."""
    eng = rig.eng.prod
    c = F.tcpcut_case(SEAM, SIZE, seam_at, strided)
    case, n = c.case, c.case.n
    case.fill(rig.a, case.raw)
    c.splace.upload(rig.a, c.src)
    rig.b.refill()
    out = eng.tcp_segment_emit(rig.a.buf, case.batch_of(), rig.a.buf, rig.b.buf, _dev(c.plans), frame_stride=c.stride,
                               out=_pre(n, 16))
    launched = eng.last_launch()
    assert launched["kernel"] == "tcpcut_kernel", launched
    got = out.cpu().numpy().reshape(-1).view(E.TCPOUT_DTYPE)
    bad = np.flatnonzero(got != c.ref_out.view(E.TCPOUT_DTYPE))
    assert bad.size == 0, (bad[:8], got[bad[:4]], c.ref_out[bad[:4]])
    rig.b.check(c.dplace.expected(c.ref_arena))
    rig.a.check(case.place.expected(case.raw) + c.splace.expected(c.src))
    print(f"far tcp_segment_emit {seam_at} stride {c.stride}: {launched['kernel']}")


@pytest.mark.parametrize("seam_at", ["inside", "end"])
def test_fragment_groups_drop_in_route_across_the_seam(rig, seam_at):
    """F.fraggroups_case, the drop-in route: emit_frag over the offloaded fragments gives the reference's
    emit-whole-then-fragment bytes (the oracle's group emit equals them); verify_frag on what the device
    emitted accepts every record, as the oracle; verify_reassemble on it delivers every datagram."""
    eng = rig.eng.prod
    c = F.fraggroups_case(SEAM, SIZE, seam_at)
    case, n, gd = c.case, c.case.n, _dev(c.groups)
    case.fill(rig.a, case.raw)
    rig.b.refill()
    est = eng.emit_frag(rig.a.buf, case.batch_of(), gd, status=_pre(n))
    assert np.array_equal(est.cpu().numpy(), c.ref_est), np.flatnonzero(est.cpu().numpy() != c.ref_est)[:8]
    rig.a.check(case.place.expected(c.emitted))
    vst = eng.verify_frag(rig.a.buf, case.batch_of(), gd, status=_pre(n)).cpu().numpy()
    assert np.array_equal(vst, c.ref_st) and (vst & E.ST_ACCEPT).all(), np.flatnonzero(vst != c.ref_st)[:8]
    st, dg = eng.verify_reassemble(rig.a.buf, case.batch_of(), gd, rig.b.buf, _dev(c.slots), status=_pre(n))
    lr = eng.last_launch()
    assert lr["kernel"] == "fragcopy_kernel", lr
    assert np.array_equal(st.cpu().numpy(), c.ref_st)
    got_dg = dg.cpu().numpy().reshape(-1).view(E.DGRAM_DTYPE)
    assert np.array_equal(got_dg, c.ref_dg), (got_dg, c.ref_dg)
    rig.b.check(c.dplace.expected(c.ref_arena))
    rig.a.check(case.place.expected(c.emitted))
    print(f"far fragment groups {seam_at}: verify_reassemble {_kv(lr)} (verify_frag / emit_frag record no launch)")


def test_nhc_udp_far_and_straddling(rig, golden):
    """F.nhc_case with the reference's own datagram (tests/golden/kat.json), against the oracle."""
    eng = rig.eng.prod
    k = golden["sixlowpan_nhc_udp"][0]
    c = F.nhc_case(SEAM, SIZE, bytes.fromhex(k["bytes"]), bytes.fromhex(k["src"]) + bytes.fromhex(k["dst"]))
    case, n, d_addrs = c.case, c.case.n, _dev(c.addrs)
    case.fill(rig.a, c.bad)
    st = eng.nhc_udp_verify(rig.a.buf, case.batch_of(), d_addrs, status=_pre(n))
    lv = eng.last_launch()
    assert np.array_equal(st.cpu().numpy(), c.ref_st), np.flatnonzero(st.cpu().numpy() != c.ref_st)[:8]
    rig.a.check(case.place.expected(c.bad))
    case.fill(rig.a, c.pre)
    est = eng.nhc_udp_emit(rig.a.buf, case.batch_of(), d_addrs, status=_pre(n))
    le = eng.last_launch()
    assert np.array_equal(est.cpu().numpy(), c.ref_est)
    rig.a.check(case.place.expected(c.after))
    print(f"far nhc_udp: verify {_kv(lv)}, emit {_kv(le)}")
