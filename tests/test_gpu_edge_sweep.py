"""GPU: the edge sweep (tests/edge_sweep.py) through every product kernel and every receive-side batched
call, compared exactly.

One corpus, placed so that every header object meets the end of every kernel's LDS window, the 64-B
segment edges and the 128-B line edges (tests/test_edge_sweep_cpu.py proves the coverage), is uploaded once
per layout and run through
  * verify and emit with every product row of variants.def forced (walk 5 / 13 / 39, tile 7, descriptor walk
    60 / 63 / 41 / 97, transposed walk 44 / 47 / 57 / 89 / 101), two caps, emit with and without
    SMOL_BATCH_FIELD_STORES, emit's input with 0xA5A5 in every checksum field;
  * the walk kernel at every launch shape (IPv4 families), the emit route and the staged transposed forms;
  * emit_fields' three forms, copy_emit 17 / 21 with copy ranges ending around the field, verify_copy,
    verify_echo_reply, verify_unreach_reply and verify_tcp_assemble.
Expected values: oracle/csum_oracle.c for status bytes and emitted buffers (sentinel bytes between the
records included), the tests/*_ref.py models for spans, entries and arenas.  last_launch() must name the
kernel of the case: a silent fallback fails.  Which kernel serves which layout is the rule `serves` below."""
import numpy as np
import pytest

import oracle
from tests import echo_ref, tcp_assemble_ref, unreach_ref
from tests import edge_sweep as S
from tests.test_verify_copy_cpu import expected_span

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from smoltcp_amd import _lib  # noqa: E402
from smoltcp_amd import engine as E  # noqa: E402
from tests.engines import VariantEngine  # noqa: E402

CAPS = [(0, 0, 0, 0, 0), (2, 3, 0, 1, 0)]
SHAPES = range(9)  # csum_launch.h CFG_*
ARENA_FILL = 0xA5  # the *_ref models' sentinel
WALK, TILE, DWALK, XWALK = "csum_kernel", "csum_tile_kernel", "dwalk_kernel", "xwalk_kernel"
FAMILY = {5: WALK, 13: WALK, 39: WALK, 7: TILE, 60: DWALK, 63: DWALK, 41: DWALK, 97: DWALK,
          44: XWALK, 47: XWALK, 57: XWALK, 89: XWALK, 101: XWALK, 80: XWALK, 81: XWALK}
PRODUCT = [5, 13, 39, 7, 60, 63, 41, 97, 44, 47, 57, 89, 101]
FIELD_TWIN = {39: 5, 47: 44, 57: 44, 89: 44, 101: 44, 97: 41, 80: 44, 81: 44}  # variants.def field_twin
VERIFY_TWIN = {41: 63, 97: 63}                                               # variants.def verify_twin
VERIFY_ONLY = {60}  # the product library carries 60's verify; its emit form is the experiments build's
DESC_FORMS, ANY_LENGTH, XWALK_FORMS = ("packed", "gaps"), ("fixed",), ("fixed2304", "fixed4032")
FORMS = DESC_FORMS + ANY_LENGTH + XWALK_FORMS


def serves(variant: int, form: str) -> bool:
    """The layouts a kernel is run on: the descriptor walk serves descriptor batches only; the transposed walk
    fixed strides of 1024-16257 B, here the two lengths that give 4 and 2 records per wavefront; the walk
    and tile kernels take any batch and get the descriptor layouts and the fixed stride just above the
    longest record."""
    fam = FAMILY[variant]
    if fam == DWALK:
        return form in DESC_FORMS
    if fam == XWALK:
        return form in XWALK_FORMS
    return form in DESC_FORMS + ANY_LENGTH


def expected_launch(variant: int, op: str, fixed: bool, field_stores: bool = False):
    v = variant
    if op == "emit" and field_stores:
        v = FIELD_TWIN.get(v, v)
    if op == "verify":
        v = VERIFY_TWIN.get(v, v)
    if v == 39 and not (op == "emit" and fixed):
        v = 5  # 39's own kernel is the fixed-stride emit; elsewhere it runs, and reports, 5
    return (TILE, 2) if FAMILY[v] == TILE else (FAMILY[v], v)


class Case:
    """One placed batch: its bytes as verify sees them, emit's input (`fill` in both bytes of every checksum
    field: 0xA5A5), the device copies (uploaded once) and the oracle's results per caps (computed once)."""

    def __init__(self, pl: S.Placed, fill: int = 0xA5):
        self.pl, self.n, self.fixed = pl, pl.n, pl.stride != 0
        self.kind, self.rflags = (int(pl.kinds[0]), int(pl.flags[0])) if self.fixed else (0, 0)  # (per record otherwise)
        self.host = pl.buf
        self.offs, self.lens = pl.offs.astype(np.int64), pl.lens.astype(np.int64)
        self.recs = [pl.record(i) for i in range(pl.n)]
        self.raw = pl.buf.copy()
        for o, r, k, f in zip(self.offs, self.recs, pl.kinds, pl.flags):
            for fo in S.field_offsets(r, int(k), int(f)):
                if fo is not None:
                    self.raw[o + fo:o + fo + 2] = fill
        self.desc = None if self.fixed else E.make_descriptors(pl.offs, pl.lens, pl.kinds, pl.flags)
        self._dev, self._ref = {}, {}

    def dev(self, name):
        if name not in self._dev:
            a = {"host": self.host, "raw": self.raw, "desc": None if self.fixed else self.desc.view(np.uint8)}[name]
            self._dev[name] = torch.from_numpy(a.copy()).to("cuda:0")
        return self._dev[name]

    def batch(self, batch_flags: int = 0):
        if self.fixed:
            return E.Batch.fixed(self.n, self.pl.stride, self.pl.length, self.kind, flags=self.rflags | batch_flags)
        return E.Batch(n=self.n, desc=self.dev("desc"), flags=batch_flags)

    def _oracle(self, fn, buf, caps):
        if self.fixed:
            return fn(buf, None, self.n, self.pl.stride, self.pl.length, oracle.kind_flags(self.kind, self.rflags), caps)
        return fn(buf, self.desc, self.n, caps=caps)

    def ref(self, caps):
        """(verify's status bytes, the emitted buffer, emit's status bytes)."""
        if caps not in self._ref:
            vst = self._oracle(oracle.batch_verify, self.host.copy(), caps)
            emitted = self.raw.copy()
            est = self._oracle(oracle.batch_emit, emitted, caps)
            if caps == CAPS[0] and self.pl.bad.any():  # the references are no trivial ones
                ok, good = (vst & E.ST_ACCEPT) != 0, (self.pl.index >= 0) & ~self.pl.bad
                assert (~ok[self.pl.bad]).sum() >= self.pl.bad.sum() // 2 and ok[good].sum() > 0.8 * good.sum()
                assert (emitted != self.raw).sum() > (self.pl.index >= 0).sum()
            self._ref[caps] = (vst, emitted, est)
        return self._ref[caps]


class Sweep:
    """The placed corpus per layout.  `corpus`: another one than the edge sweep's, `case`: what wraps a placement
    (tests/test_gpu_sum_sweep.py).  Records longer than S.LMAX, of which the edge sweep's corpus has none, are for
    the two descriptor layouts only: place_fixed would cut them.  `limit`: the largest fixed-stride buffer; above
    it place_fixed gives up records that meet no new edge cell."""

    def __init__(self, corpus=None, case=Case, limit=64 << 20):
        self.corpus = S.build_corpus() if corpus is None else corpus
        self.case, self.limit = case, limit
        self.short = [r for r in self.corpus if len(r.data) <= S.LMAX]
        # what verify_tcp_assemble is given: see test_verify_tcp_assemble
        self.tcp_corpus = [r for r in self.short if S.geometry(r.data, r.kind, emit=True).proto == S.P_TCP]
        self._forms = {}

    def cases(self, form):
        if form not in self._forms:
            c = self.short
            both = [(k, f) for k in (S.KIND_IP, S.KIND_ETH) for f in (0, S.REC_IPHDR_ONLY) if any(r.flags == f for r in c)]
            v4 = [r for r in c if r.family.startswith("v4/")]
            if form in DESC_FORMS:
                pls = [S.place_desc(self.corpus, gaps=form == "gaps")]
            elif form == "fixed":
                pls = [S.place_fixed(c, k, f) for k, f in both]
            elif form == "fixed2304":
                pls = [S.place_fixed(c, k, f, 2304, 2305, limit=self.limit) for k, f in both]
            elif form == "fixed4032":
                pls = [S.place_fixed(c, k, 0, 4032, 4033, limit=self.limit) for k in (S.KIND_IP, S.KIND_ETH)]
            elif form == "route":  # see test_emit_route
                pls = [S.place_fixed(c, k, 0, S.LMAX + 1, S.LMAX + 1) for k in (S.KIND_IP, S.KIND_ETH)]
            elif form == "v4gaps":
                pls = [S.place_desc(v4, gaps=True)]
            elif form == "v4fixed":
                L = max(len(r.data) for r in v4)
                pls = [S.place_fixed(v4, k, 0, L, L + 1 + L % 2) for k in (S.KIND_IP, S.KIND_ETH)]
            elif form == "tcpgaps":
                pls = [S.place_desc(self.tcp_corpus, gaps=True)]
            elif form == "tcpfixed":
                pls = [S.place_fixed(self.tcp_corpus, k, 0) for k in (S.KIND_IP, S.KIND_ETH)]
            self._forms[form] = [self.case(pl) for pl in pls]
        return self._forms[form]


@pytest.fixture(scope="module")
def sweep():
    return Sweep()


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    e = VariantEngine(0)
    yield e
    e.close()


def _same(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: differs at {bad[:8]}: got {got[bad[:8]]} want {want[bad[:8]]}"


def _where(case, pos):
    """The record (index, offset in it, family) a buffer position belongs to, for a failure's message."""
    i = int(np.searchsorted(case.offs, pos, side="right")) - 1
    j = int(case.pl.index[i]) if i >= 0 else -1
    return i, int(pos - case.offs[i]), int(case.offs[i] % 128), "filler" if j < 0 else j


def _verify_emit(eng, case, variant, caps, tag, want_v=None, want_e=None, field_stores=(False, True), verify=True):
    """verify and emit of one case under the engine's current settings, against the oracle."""
    vst, emitted, est = case.ref(caps)
    if verify:
        st = eng.verify(case.dev("host"), case.batch(), caps=caps).cpu().numpy()
        lv = eng.last_launch()
        if want_v:
            assert (lv["kernel"], lv["variant"]) == want_v, (tag, "verify", lv)
        _same(st, vst, f"{tag} caps {caps}: verify status")
    for fs in field_stores if variant not in VERIFY_ONLY else ():
        d = case.dev("raw").clone()
        status = torch.zeros(case.n, dtype=torch.uint8, device="cuda:0")
        eng.emit(d, case.batch(E.BATCH_FIELD_STORES if fs else 0), caps=caps, status=status)
        le = eng.last_launch()
        if want_e:
            assert (le["kernel"], le["variant"]) == want_e[fs], (tag, "emit", fs, le)
        got = d.cpu().numpy()
        diff = np.flatnonzero(got != emitted)
        assert diff.size == 0, (f"{tag} caps {caps} field stores {fs}: emitted bytes differ at {diff[:8]}, record / offset / "
                                f"start mod 128 / corpus index {[_where(case, p) for p in diff[:4]]}")
        _same(status.cpu().numpy(), est, f"{tag} caps {caps} field stores {fs}: emit status")


# ---------------------------------------------------------------------------------------------
# verify and emit: every product kernel on every layout it serves
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("variant,form", [(v, f) for v in PRODUCT for f in FORMS if serves(v, f)])
def test_verify_and_emit(eng, sweep, variant, form):
    assert eng.prod.variant_built(variant), "a product row of variants.def"
    eng.set_variant(variant)
    try:
        assert eng.cur is eng.prod
        for case in sweep.cases(form):
            tag = (variant, form, case.kind, case.rflags)
            want_v = expected_launch(variant, "verify", case.fixed)
            want_e = {fs: expected_launch(variant, "emit", case.fixed, fs) for fs in (False, True)}
            for caps in CAPS:
                _verify_emit(eng, case, variant, caps, tag, want_v, want_e)
    finally:
        eng.set_variant(-1)


@pytest.mark.parametrize("form", FORMS)
def test_the_library_s_own_choice(eng, sweep, form):
    """Nothing forced: the dispatch's pick for each layout (kernel_for names it) gives the oracle's results."""
    for case in sweep.cases(form):
        want_v, want_e = eng.kernel_for("verify", case.batch()), eng.kernel_for("emit", case.batch())
        vst, emitted, est = case.ref(CAPS[0])
        st = eng.verify(case.dev("host"), case.batch()).cpu().numpy()
        assert eng.last_launch()["kernel"] == want_v
        _same(st, vst, f"{form}: verify status")
        d = case.dev("raw").clone()
        eng.emit(d, case.batch())
        assert eng.last_launch()["kernel"] == want_e
        _same(d.cpu().numpy(), emitted, f"{form}: emitted bytes")


@pytest.mark.parametrize("form", ["v4gaps", "v4fixed"])
@pytest.mark.parametrize("variant", [5, 13, 39])
def test_walk_kernel_every_shape(eng, sweep, variant, form):
    """The walk kernel's forms at each of its launch shapes over the IPv4 families (IHL 5..15, every L4
    protocol, the ICMPv4 errors' embedded headers, the raw-socket twins)."""
    eng.set_variant(variant)
    try:
        for shape in SHAPES:
            eng.set_shape(shape)
            for case in sweep.cases(form):
                want_v = expected_launch(variant, "verify", case.fixed)
                want_e = {fs: expected_launch(variant, "emit", case.fixed, fs) for fs in (False, True)}
                _verify_emit(eng, case, variant, CAPS[0], (variant, form, shape, case.kind), want_v, want_e)
    finally:
        eng.set_shape(-1)
        eng.set_variant(-1)


def test_emit_route(eng, sweep):
    """The two-launch emit route, forced wherever it is legal.  The route takes what the dispatch table picks
    by itself when that is 57 or 101; at 2304 B the table's row gives those to packed strides only (its
    gapped column is 47), and a packed stride of 2304 B puts every record at one start residue.  So the
    sweep runs the route at 2201 B packed: an odd stride (all 128 residues), just above the longest record,
    where the table's row takes 57."""
    eng.set_emit_route(1)
    try:
        for case in sweep.cases("route"):
            for caps in CAPS:
                _, emitted, est = case.ref(caps)
                d = case.dev("raw").clone()
                status = torch.zeros(case.n, dtype=torch.uint8, device="cuda:0")
                eng.emit(d, case.batch(), caps=caps, status=status)
                assert eng.last_route(), "the route did not run"
                le = eng.last_launch()
                assert (le["kernel"], le["variant"]) == (XWALK, 57), le
                got = d.cpu().numpy()
                diff = np.flatnonzero(got != emitted)
                assert diff.size == 0, (caps, diff[:8], [_where(case, p) for p in diff[:4]])
                _same(status.cpu().numpy(), est, "route: emit status")
    finally:
        eng.set_emit_route(-1)


@pytest.mark.parametrize("variant", [80, 81])
def test_staged_transposed_emit(eng, sweep, variant):
    """The staged transposed forms (experiments build) at 2304 B: field entries, then the segment pass."""
    eng.need(variant)
    eng.set_variant(variant)
    try:
        for case in sweep.cases("fixed2304"):
            want_e = {fs: expected_launch(variant, "emit", True, fs) for fs in (False, True)}
            for caps in CAPS:
                _verify_emit(eng, case, variant, caps, (variant, case.kind, case.rflags), None, want_e, verify=False)
    finally:
        eng.set_variant(-1)


# ---------------------------------------------------------------------------------------------
# emit_fields
# ---------------------------------------------------------------------------------------------

FK_WALK, FK_XWALK, FK_DWALK = 1, 2, 3
FIELDS_KERNEL = {FK_WALK: "csum_fields_kernel", FK_XWALK: "xwalk_kernel(fields)", FK_DWALK: "dwalk_kernel(fields)"}
FIELDS_FORMS = {FK_WALK: DESC_FORMS + ANY_LENGTH + ("fixed2304",), FK_XWALK: XWALK_FORMS, FK_DWALK: DESC_FORMS}


@pytest.mark.parametrize("kernel,form", [(k, f) for k in (FK_WALK, FK_XWALK, FK_DWALK) for f in FIELDS_FORMS[k]])
def test_emit_fields(eng, sweep, kernel, form):
    """The entries applied to the host copy give the oracle's emit; the device buffer is only read."""
    e = eng.prod
    e.set_fields_kernel(kernel)
    try:
        for case in sweep.cases(form):
            for caps in CAPS:
                _, emitted, est = case.ref(caps)
                ent = torch.full((case.n + 8, 16), 0xA5, dtype=torch.uint8, device="cuda:0")
                e.emit_fields(case.dev("raw"), case.batch(), caps=caps, fields=ent)
                assert e.last_launch()["kernel"] == FIELDS_KERNEL[kernel], e.last_launch()
                got = ent.cpu().numpy()
                assert (got[case.n:] == 0xA5).all(), "entries past n written"
                f = got[:case.n].reshape(-1).view(E.FIELDS_DTYPE)
                patched = case.raw.copy()
                ok = E.apply_fields(patched, case.offs, case.lens, f)
                assert ok.all(), np.flatnonzero(~ok)[:8]
                diff = np.flatnonzero(patched != emitted)
                assert diff.size == 0, (form, caps, diff[:8], [_where(case, p) for p in diff[:4]])
                _same(f["status"], est, "entry status")
                none = f["off"] == _lib.NO_FIELD
                assert (f["val"][none] == 0).all() and not f["reserved"].any()
            assert torch.equal(case.dev("raw"), torch.from_numpy(case.raw).to("cuda:0")), "the device buffer changed"
    finally:
        e.set_fields_kernel(0)


# ---------------------------------------------------------------------------------------------
# copy_emit
# ---------------------------------------------------------------------------------------------

# where the copy range ends: the whole L4 payload (an ICMPv4 error's covers the embedded header's field, every
# other one starts behind the L4 field), or from the L4 header's first byte to d bytes past the L4 field's first
# byte: one byte short of it, on it, its first byte only, the whole field, one byte more
COPY_ENDS = ("payload", -1, 0, 1, 2, 3)


def _copy_plan(case, end, rng):
    """(source buffer, copy descriptors) of one copy_emit call.  The source holds fresh random payload bytes;
    header bytes in a range are the record's own (the caller wrote the headers already) except a random
    source port, and every checksum field inside a range holds 0x3C3C: the emitted field wins."""
    chunks, so, do, ln, pos = [], [], [], [], 0
    for rec, k, fl in zip(case.recs, case.pl.kinds, case.pl.flags):
        g = S.geometry(rec, int(k), int(fl), emit=True)
        a = b = 0
        if not g.malformed and g.proto:
            f, e = g.l4_off + S.L4_FIELD[g.proto], S.span_end(rec, g)
            if end == "payload":
                a = g.l4_off + ((rec[g.l4_off + 12] >> 4) * 4 if g.proto == S.P_TCP else 8)
                b = max(a, e)
            else:
                a, b = g.l4_off, min(f + end, e)
        data = bytearray(rec[a:b])
        if end == "payload":
            emb = S.embedded_header(rec, g)
            keep = emb[1] if emb else 0  # an embedded header stays (its length rules the geometry)
            data[keep:] = rng.integers(0, 256, len(data) - keep, dtype=np.uint8).tobytes()
        elif len(data) >= 2 and g.proto in (S.P_UDP, S.P_TCP):
            data[0:2] = bytes([int(rng.integers(1, 256)), int(rng.integers(0, 256))])
        for fo in S.field_offsets(rec, int(k), int(fl)):
            for j in (0, 1):
                if fo is not None and a <= fo + j < b:
                    data[fo + j - a] = 0x3C
        pad = int(rng.integers(0, 4))
        chunks.append(bytes(pad) + bytes(data))
        so.append(pos + pad), do.append(a), ln.append(b - a)
        pos += pad + len(data)
    src = np.frombuffer(b"".join(chunks) + bytes(16), np.uint8).copy()
    return src, E.make_copies(np.array(so, np.uint64), np.array(do, np.uint32), np.array(ln, np.uint32))


@pytest.mark.parametrize("form", ["gaps", "packed", "fixed"])
@pytest.mark.parametrize("variant", [17, 21])
def test_copy_emit(eng, sweep, variant, form):
    """memcpy followed by the oracle's emit, for copy ranges that cover, touch and stop short of the field."""
    rng = np.random.default_rng(variant)
    eng.set_variant(variant)
    try:
        for case in sweep.cases(form):
            if case.rflags:
                continue  # a raw-socket frame's L4 bytes are the user's: nothing to copy behind its headers
            for end in COPY_ENDS:
                src, copies = _copy_plan(case, end, rng)
                ref = case.raw.copy()
                if case.fixed:
                    rst = oracle.batch_copy_emit(ref, None, case.n, src, copies, case.pl.stride, case.pl.length, case.kind)
                else:
                    rst = oracle.batch_copy_emit(ref, case.desc, case.n, src, copies)
                d = case.dev("raw").clone()
                status = torch.zeros(case.n, dtype=torch.uint8, device="cuda:0")
                eng.copy_emit(d, case.batch(), torch.from_numpy(src).cuda(), torch.from_numpy(copies.view(np.uint8).copy()).cuda(),
                              status=status)
                lc = eng.last_launch()
                assert (lc["kernel"], lc["variant"]) == ("copy_kernel", variant), lc
                got = d.cpu().numpy()
                diff = np.flatnonzero(got != ref)
                assert diff.size == 0, (variant, form, end, diff[:8], [_where(case, p) for p in diff[:4]])
                _same(status.cpu().numpy(), rst, f"copy_emit {variant} {form} {end}: status")
    finally:
        eng.set_variant(-1)


# ---------------------------------------------------------------------------------------------
# The receive-side batched calls
# ---------------------------------------------------------------------------------------------

# the shapes vcopy_shape (csum_dispatch.h) returns: 8 x 7 over descriptors; over fixed strides 8 x 6 up to
# 1521 B, 32 x 4 up to 2033 B, 64 x 4 above (the layout's 2200 B: the automatic one), each forced in turn there
RX_FORMS = [("gaps", -1), ("packed", -1), ("fixed", -1), ("fixed", 0), ("fixed", 4)]
RX_SHAPE = {("gaps", -1): (8, 7), ("packed", -1): (8, 7), ("fixed", -1): (64, 4), ("fixed", 0): (8, 6), ("fixed", 4): (32, 4)}


def _rx_cases(sweep, form):
    return [c for c in sweep.cases(form) if not c.rflags or not c.fixed]


def _slots(lens, rng):
    """Slots back to back at shuffled residues: slot i holds lens[i] bytes exactly."""
    offs, pos = np.zeros(len(lens), np.uint64), 5
    for i, n in enumerate(lens):
        pos += int(rng.integers(0, 3)) if n else 0
        offs[i] = pos
        pos += int(n)
    return E.make_slots(offs, np.asarray(lens, np.uint32)), pos + 37


def _launched(eng, kernel, form, shape):
    l = eng.last_launch()
    assert l["kernel"] == kernel and (l["G"], l["U"]) == RX_SHAPE[(form, shape)], l


@pytest.mark.parametrize("form,shape", RX_FORMS)
def test_verify_copy(eng, sweep, form, shape):
    rng = np.random.default_rng(3)
    e = eng.prod
    e.set_shape(shape)
    try:
        for case in _rx_cases(sweep, form):
            vst = case.ref(CAPS[0])[0]
            spans = [expected_span(r, int(k), int(f)) for r, k, f in zip(case.recs, case.pl.kinds, case.pl.flags)]
            slots, size = _slots([sp[1] if sp else 0 for sp in spans], rng)
            arena = np.full(size, ARENA_FILL, np.uint8)
            ref_sp = np.zeros(case.n, E.SPAN_DTYPE)
            for i, sp in enumerate(spans):
                if sp:
                    ref_sp[i] = (sp[1], sp[0], 1, 0)
                    o = int(slots["dst_offset"][i])
                    arena[o:o + sp[1]] = np.frombuffer(case.recs[i][sp[0]:sp[0] + sp[1]], np.uint8)
            dst = torch.full((size,), ARENA_FILL, dtype=torch.uint8, device="cuda:0")
            st, sp = e.verify_copy(case.dev("host"), case.batch(), dst, torch.from_numpy(slots.view(np.uint8).copy()).cuda())
            _launched(e, "vcopy_kernel", form, shape)
            _same(st.cpu().numpy(), vst, "verify_copy status")
            _same(sp.cpu().numpy().reshape(-1).view(E.SPAN_DTYPE), ref_sp, "spans")
            _same(dst.cpu().numpy(), arena, "arena")
            assert sum(1 for s in spans if s and s[0] > 128) > 100  # payloads behind the 128-B window
    finally:
        e.set_shape(-1)


@pytest.mark.parametrize("form,shape", RX_FORMS)
def test_verify_echo_reply(eng, sweep, form, shape):
    rng = np.random.default_rng(4)
    e = eng.prod
    e.set_shape(shape)
    try:
        for case in _rx_cases(sweep, form):
            need = echo_ref.frame_lens(case.recs, case.pl.kinds, case.pl.flags, None)
            slots, size = _slots(need, rng)
            st, ent, arena = echo_ref.expected(case.recs, case.pl.kinds, case.pl.flags, CAPS[0], None, slots, size)
            _same(st, case.ref(CAPS[0])[0], "the model's status and verify's")
            dst = torch.full((size,), ARENA_FILL, dtype=torch.uint8, device="cuda:0")
            gst, gent = e.verify_echo_reply(case.dev("host"), case.batch(), dst, torch.from_numpy(slots.view(np.uint8).copy()).cuda())
            _launched(e, "echo", form, shape)
            _same(gst.cpu().numpy(), st, "verify_echo_reply status")
            _same(gent.cpu().numpy().reshape(-1).view(E.ECHO_DTYPE), ent, "entries")
            _same(dst.cpu().numpy(), arena, "arena")
            assert (ent["data_off"][(ent["flags"] & E.ECHO_WRITTEN) != 0] > 128).sum() > 50  # requests behind the window
    finally:
        e.set_shape(-1)


@pytest.mark.parametrize("form,shape", RX_FORMS)
def test_verify_unreach_reply(eng, sweep, form, shape):
    rng = np.random.default_rng(5)
    e = eng.prod
    port_map = E.make_port_map(set(range(1, 6000)) - set(S.CLOSED_PORTS))
    e.set_shape(shape)
    try:
        for case in _rx_cases(sweep, form):
            need = unreach_ref.frame_lens(case.recs, case.pl.kinds, case.pl.flags, port_map, None)
            slots, size = _slots(need, rng)
            st, ent, arena = unreach_ref.expected(case.recs, case.pl.kinds, case.pl.flags, CAPS[0], None, port_map, slots, size)
            _same(st, case.ref(CAPS[0])[0], "the model's status and verify's")
            dst = torch.full((size,), ARENA_FILL, dtype=torch.uint8, device="cuda:0")
            gst, gent = e.verify_unreach_reply(case.dev("host"), case.batch(), dst,
                                               torch.from_numpy(slots.view(np.uint8).copy()).cuda(), torch.from_numpy(port_map).cuda())
            _launched(e, "unreach", form, shape)
            _same(gst.cpu().numpy(), st, "verify_unreach_reply status")
            _same(gent.cpu().numpy().reshape(-1).view(E.UNR_DTYPE), ent, "entries")
            _same(dst.cpu().numpy(), arena, "arena")
            written = (ent["flags"] & E.UNR_WRITTEN) != 0
            assert written.sum() > 300 and (ent["flags"][written] & E.UNR_PORT).any()
    finally:
        e.set_shape(-1)


@pytest.mark.parametrize("form", ["tcpgaps", "tcpfixed"])
def test_verify_tcp_assemble(eng, sweep, form):
    """One connection per 64 records of the corpus's TCP records, placed at their start residues with gaps and
    at a fixed stride (whose fillers carry no segment).  The sequence numbers are rewritten so that a group's
    payloads follow one another, the checksums filled again and the bad-checksum copies' bytes flipped again;
    the window takes everything and each ring holds its group's payloads exactly."""
    e = eng.prod
    for case in sweep.cases(form):
        pl, n = case.pl, case.n
        buf = case.host.copy()
        groups = [(a, min(64, n - a), 0) for a in range(0, n, 64)]
        ring, ws = [], 0xFFFFF000  # (the sequence numbers wrap)
        for a, c, _ in groups:
            seq = ws
            for i in range(a, a + c):
                t = tcp_assemble_ref.tcp_segment(case.recs[i], int(pl.kinds[i]), int(pl.flags[i]))
                if t is not None:
                    g = S.geometry(case.recs[i], int(pl.kinds[i]), int(pl.flags[i]))
                    o = int(case.offs[i]) + g.l4_off + 4
                    buf[o:o + 4] = np.frombuffer((seq & 0xFFFFFFFF).to_bytes(4, "big"), np.uint8)
                    seq += t[1]
            ring.append(seq - ws)
        case._oracle(oracle.batch_emit, buf, CAPS[0])
        for i in np.flatnonzero(pl.bad):
            r = sweep.tcp_corpus[int(pl.index[i])]
            buf[int(case.offs[i]) + S.flip_offsets(r.data, r.kind, r.flags)[r.bad]] ^= 0x5A
        recs = [buf[int(o):int(o + ln)].tobytes() for o, ln in zip(case.offs, case.lens)]
        vst = case._oracle(oracle.batch_verify, buf.copy(), CAPS[0])
        assert 50 < ((vst & E.ST_ACCEPT) == 0).sum() < n // 2
        base = 7 + np.concatenate([[0], np.cumsum(np.array(ring[:-1], np.int64) + 3)])
        wins = E.make_tcpwins(base, ring, 0, ws, ring)
        size = int(base[-1]) + ring[-1] + 29
        segs, flows, arena, written = tcp_assemble_ref.expected(recs, pl.kinds, pl.flags, groups, wins, (vst & E.ST_ACCEPT) != 0,
                                                                size)
        copied = (segs["flags"] & tcp_assemble_ref.SEG_COPIED) != 0
        assert written.all() and copied.sum() > 1000
        assert (segs["off"][copied] > 128).sum() > 100  # payloads behind the 128-B window
        dst = torch.full((size,), ARENA_FILL, dtype=torch.uint8, device="cuda:0")
        gd = torch.from_numpy(E.make_groups([g[0] for g in groups], [g[1] for g in groups]).view(np.uint8).copy()).cuda()
        st, gs, gf = e.verify_tcp_assemble(torch.from_numpy(buf).cuda(), case.batch(), gd, dst,
                                           torch.from_numpy(wins.view(np.uint8).copy()).cuda())
        assert e.last_launch()["kernel"] == "tcpasm_kernel", e.last_launch()
        _same(st.cpu().numpy(), vst, "verify_tcp_assemble status")
        _same(gs.cpu().numpy().reshape(-1).view(E.TCPSEG_DTYPE), segs, "segments")
        _same(gf.cpu().numpy().reshape(-1).view(E.TCPFLOW_DTYPE), flows, "flows")
        _same(dst.cpu().numpy(), arena, "rings")
