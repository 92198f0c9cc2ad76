"""GPU: the sum sweep (tests/sum_sweep.py) through every kernel, compared exactly.

The edge sweep's rig (tests/test_gpu_edge_sweep.py: Sweep, Case, the layouts, `serves`, `expected_launch`) over a
corpus whose sums lie on the values where one's-complement arithmetic breaks: both zeros and their neighbours,
all-zero spans, sums that are a multiple of 0xffff in the data or in the pseudo-header alone, header checksums
of 0x0000, the SMOL_ST_L4_PARTIAL comparison, and records long enough to set bit 31 of a u32 accumulator
(tests/test_sum_sweep_cpu.py proves that every class reaches every family, and that nine kinds of wrong
arithmetic are noticed).  Emit runs over four contents of the checksum fields (0x0000, 0xffff, 0xA5A5, the right
value): a kernel that takes the old content off a sum meets each class with each.

Expected values: oracle/csum_oracle.c for status bytes and emitted buffers, the tests/*_ref.py models for
spans, entries and arenas.  last_launch() must name the kernel of the case."""
import numpy as np
import pytest

import oracle
from tests import echo_ref, tcp_assemble_ref, tcp_segment_ref, unreach_ref
from tests import edge_sweep as S
from tests import pktgen as P
from tests import sum_sweep as Q
from tests import udp_enqueue_ref as R
from tests.test_verify_copy_cpu import expected_span

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from smoltcp_amd import engine as E  # noqa: E402
from tests.test_gpu_edge_sweep import (ARENA_FILL, CAPS, DESC_FORMS, FIELDS_FORMS, FIELDS_KERNEL, FORMS, PRODUCT, RX_FORMS,  # noqa: E402,F401
                                       SHAPES, XWALK, Case, Sweep, _launched, _rx_cases, _same, _slots, _where, eng,
                                       expected_launch, serves)

FILLS = {"0000": 0x00, "ffff": 0xFF, "a5a5": 0xA5, "kept": None}  # both bytes of every checksum field before emit


class SumCase(Case):
    """A placed batch with emit's input under each fill ("kept": what the corpus holds, the right value on all but
    the verify copies), and the expected results on the device."""

    def __init__(self, pl):
        super().__init__(pl)  # self.raw: 0xA5A5
        at = np.array([o + fo for o, r, k in zip(self.offs, self.recs, pl.kinds) for fo in S.field_offsets(r, int(k)) if fo is not None])
        self.raws = {"a5a5": self.raw, "kept": self.host}
        for name in ("0000", "ffff"):
            self.raws[name] = self.host.copy()
            self.raws[name][at] = self.raws[name][at + 1] = FILLS[name]
        assert (self.raw[at] == 0xA5).all() and at.size >= self.n

    def dev(self, name):
        if name in self.raws and name not in self._dev:
            self._dev[name] = torch.from_numpy(self.raws[name].copy()).to("cuda:0")
        return self._dev[name] if name in self._dev else super().dev(name)

    def ref(self, caps):
        """The edge sweep's (verify status, emitted buffer, emit status); emit's result is the same under every
        fill (the oracle run on each), and is kept on the device too."""
        if caps not in self._ref:
            vst, emitted, est = super().ref(caps)
            for name in ("0000", "ffff", "kept"):
                again = self.raws[name].copy()
                assert np.array_equal(self._oracle(oracle.batch_emit, again, caps), est) and np.array_equal(again, emitted), name
            self._dev[("emitted", caps)] = torch.from_numpy(emitted).to("cuda:0")
        return self._ref[caps]

    def emitted_dev(self, caps):
        self.ref(caps)
        return self._dev[("emitted", caps)]


@pytest.fixture(scope="module")
def sweep():
    # (96 MiB: at 4033 B a start residue's 130 records need 68 MiB, and every record of this corpus is there for its sums)
    sw = Sweep(Q.build_corpus(), SumCase, limit=96 << 20)
    assert 3000 <= len(sw.corpus) <= 8862
    return sw


def _check_emitted(case, d, caps, what):
    """The emitted buffer against the oracle's, compared on the device; a difference is located on the host."""
    if not torch.equal(d, case.emitted_dev(caps)):
        diff = np.flatnonzero(d.cpu().numpy() != case.ref(caps)[1])
        raise AssertionError(f"{what} caps {caps}: emitted bytes differ at {diff[:8]}, record / offset / start mod 128 / corpus "
                             f"index {[_where(case, p) for p in diff[:4]]}")


def _verify_emit(eng, case, variant, caps, tag, want_v=None, want_e=None, verify=True, fills=FILLS):
    """verify, and emit over each fill with and without SMOL_BATCH_FIELD_STORES, against the oracle."""
    vst, _, est = case.ref(caps)
    if verify:
        st = eng.verify(case.dev("host"), case.batch(), caps=caps).cpu().numpy()
        lv = eng.last_launch()
        if want_v:
            assert (lv["kernel"], lv["variant"]) == want_v, (tag, "verify", lv)
        _same(st, vst, f"{tag} caps {caps}: verify status")
    for fs in (False, True) if variant != 60 else ():  # (60: the product library carries its verify only)
        for fill in fills:
            d = case.dev(fill).clone()
            status = torch.zeros(case.n, dtype=torch.uint8, device="cuda:0")
            eng.emit(d, case.batch(E.BATCH_FIELD_STORES if fs else 0), caps=caps, status=status)
            le = eng.last_launch()
            if want_e:
                assert (le["kernel"], le["variant"]) == want_e[fs], (tag, "emit", fs, le)
            _check_emitted(case, d, caps, f"{tag} field stores {fs} fill {fill}")
            _same(status.cpu().numpy(), est, f"{tag} caps {caps} field stores {fs} fill {fill}: emit status")


# ---------------------------------------------------------------------------------------------
# verify and emit: every product kernel on every layout it serves
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("variant,form", [(v, f) for v in PRODUCT for f in FORMS if serves(v, f)])
def test_verify_and_emit(eng, sweep, variant, form):
    assert eng.prod.variant_built(variant), "a product row of variants.def"
    eng.set_variant(variant)
    try:
        assert eng.cur is eng.prod
        placed = sum(int((case.pl.index >= 0).sum()) for case in sweep.cases(form))
        assert placed == len(sweep.corpus if form in DESC_FORMS else sweep.short), "a layout gave records up"
        for case in sweep.cases(form):
            tag = (variant, form, case.kind)
            want_v = expected_launch(variant, "verify", case.fixed)
            want_e = {fs: expected_launch(variant, "emit", case.fixed, fs) for fs in (False, True)}
            for caps in CAPS:
                _verify_emit(eng, case, variant, caps, tag, want_v, want_e)
    finally:
        eng.set_variant(-1)


@pytest.mark.parametrize("form", FORMS)
def test_the_library_s_own_choice(eng, sweep, form):
    for case in sweep.cases(form):
        want_v, want_e = eng.kernel_for("verify", case.batch()), eng.kernel_for("emit", case.batch())
        vst, _, est = case.ref(CAPS[0])
        st = eng.verify(case.dev("host"), case.batch()).cpu().numpy()
        assert eng.last_launch()["kernel"] == want_v
        _same(st, vst, f"{form}: verify status")
        for fill in FILLS:
            d = case.dev(fill).clone()
            eng.emit(d, case.batch())
            assert eng.last_launch()["kernel"] == want_e
            _check_emitted(case, d, CAPS[0], f"{form} fill {fill}")


@pytest.mark.parametrize("form", ["v4gaps", "v4fixed"])
@pytest.mark.parametrize("variant", [5, 13, 39])
def test_walk_kernel_every_shape(eng, sweep, variant, form):
    """The walk kernel's forms at each of its launch shapes over the IPv4 families: H0 and IN0, ZERO, the L4 classes
    behind 20 and 60 header bytes."""
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
    """The two-launch emit route at 2201 B packed (see the edge sweep's test), each fill."""
    eng.set_emit_route(1)
    try:
        for case in sweep.cases("route"):
            for caps in CAPS:
                est = case.ref(caps)[2]
                for fill in FILLS:
                    d = case.dev(fill).clone()
                    status = torch.zeros(case.n, dtype=torch.uint8, device="cuda:0")
                    eng.emit(d, case.batch(), caps=caps, status=status)
                    assert eng.last_route(), "the route did not run"
                    le = eng.last_launch()
                    assert (le["kernel"], le["variant"]) == (XWALK, 57), le
                    _check_emitted(case, d, caps, f"route fill {fill}")
                    _same(status.cpu().numpy(), est, "route: emit status")
    finally:
        eng.set_emit_route(-1)


@pytest.mark.parametrize("variant", [80, 81])
def test_staged_transposed_emit(eng, sweep, variant):
    eng.need(variant)
    eng.set_variant(variant)
    try:
        for case in sweep.cases("fixed2304"):
            want_e = {fs: expected_launch(variant, "emit", True, fs) for fs in (False, True)}
            for caps in CAPS:
                _verify_emit(eng, case, variant, caps, (variant, case.kind), None, want_e, verify=False)
    finally:
        eng.set_variant(-1)


@pytest.mark.parametrize("variant", [44, 47, 57, 89, 101])
def test_transposed_walk_headroom(eng, variant):
    """The transposed walk's longest records (16257 B, one per wavefront), every free byte 0xff, back to back at an
    odd stride: the largest sums its lanes and its per-record reduction meet."""
    recs, wrong = Q.xwalk_headroom()
    L = Q.XWALK_LONGEST
    host = np.frombuffer(b"".join(recs) + bytes([S.SENTINEL]) * 144, np.uint8).copy()
    n = len(recs)
    batch = E.Batch.fixed(n, L, L, E.KIND_ETH)
    raw = {name: host.copy() for name in FILLS}
    for name, fill in FILLS.items():
        if fill is not None:
            raw[name][:n * L].reshape(n, L)[:, 70:72] = fill
    eng.set_variant(variant)
    try:
        for caps in CAPS:
            vst = oracle.batch_verify(host.copy(), None, n, L, L, E.KIND_ETH, caps)
            assert ((vst & E.ST_ACCEPT) == 0).tolist() == [w and caps[2] in (0, 1) for w in wrong]
            st = eng.verify(torch.from_numpy(host).cuda(), batch, caps=caps).cpu().numpy()
            lv = eng.last_launch()
            assert (lv["kernel"], lv["variant"]) == expected_launch(variant, "verify", True), lv
            _same(st, vst, f"{variant} caps {caps}: verify status")
            for fs in (False, True):
                for name in FILLS:
                    want = raw[name].copy()
                    est = oracle.batch_emit(want, None, n, L, L, E.KIND_ETH, caps)
                    d = torch.from_numpy(raw[name]).cuda()
                    status = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
                    eng.emit(d, E.Batch.fixed(n, L, L, E.KIND_ETH, flags=E.BATCH_FIELD_STORES if fs else 0), caps=caps, status=status)
                    le = eng.last_launch()
                    assert (le["kernel"], le["variant"]) == expected_launch(variant, "emit", True, fs), le
                    _same(d.cpu().numpy(), want, f"{variant} caps {caps} field stores {fs} fill {name}: emitted bytes")
                    _same(status.cpu().numpy(), est, "emit status")
    finally:
        eng.set_variant(-1)


# ---------------------------------------------------------------------------------------------
# emit_fields, copy_emit
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kernel,form", [(k, f) for k in FIELDS_KERNEL for f in FIELDS_FORMS[k]])
def test_emit_fields(eng, sweep, kernel, form):
    e = eng.prod
    e.set_fields_kernel(kernel)
    try:
        for case in sweep.cases(form):
            for caps in CAPS:
                _, emitted, est = case.ref(caps)
                for fill in FILLS:
                    ent = torch.full((case.n + 8, 16), 0xA5, dtype=torch.uint8, device="cuda:0")
                    e.emit_fields(case.dev(fill), case.batch(), caps=caps, fields=ent)
                    assert e.last_launch()["kernel"] == FIELDS_KERNEL[kernel], e.last_launch()
                    got = ent.cpu().numpy()
                    assert (got[case.n:] == 0xA5).all(), "entries past n written"
                    f = got[:case.n].reshape(-1).view(E.FIELDS_DTYPE)
                    patched = case.raws[fill].copy()
                    ok = E.apply_fields(patched, case.offs, case.lens, f)
                    assert ok.all(), np.flatnonzero(~ok)[:8]
                    diff = np.flatnonzero(patched != emitted)
                    assert diff.size == 0, (form, caps, fill, diff[:8], [_where(case, p) for p in diff[:4]])
                    _same(f["status"], est, "entry status")
    finally:
        e.set_fields_kernel(0)


@pytest.mark.parametrize("form", ["gaps", "packed", "fixed"])
@pytest.mark.parametrize("variant", [17, 21])
def test_copy_emit(eng, sweep, variant, form):
    """Each record's bytes behind its L4 field's word come from a source buffer (the record's own, so the sums keep
    their class) over a destination that holds their complement there; each fill in the fields."""
    eng.set_variant(variant)
    try:
        for case in sweep.cases(form):
            so, do, ln, chunks, pos = [], [], [], [], 0
            scrambled = {name: case.raws[name].copy() for name in FILLS}
            for o, rec, k in zip(case.offs, case.recs, case.pl.kinds):
                g = S.geometry(rec, int(k), emit=True)
                a = g.l4_off + S.L4_FIELD[g.proto] + 2 if g.gate else 0
                b = S.span_end(rec, g) if g.gate else 0
                pad = (len(so) * 7) % 4
                chunks.append(bytes(pad) + rec[a:b])
                so.append(pos + pad), do.append(a), ln.append(b - a)
                pos += pad + b - a
                for name in FILLS:  # (an embedded header's field lies in the range: the copy brings the source's, emit fills it)
                    scrambled[name][o + a:o + b] ^= 0xFF
            src = np.frombuffer(b"".join(chunks) + bytes(16), np.uint8).copy()
            copies = E.make_copies(np.array(so, np.uint64), np.array(do, np.uint32), np.array(ln, np.uint32))
            d_src, d_copies = torch.from_numpy(src).cuda(), torch.from_numpy(copies.view(np.uint8).copy()).cuda()
            for name in FILLS:
                ref = scrambled[name].copy()
                if case.fixed:
                    rst = oracle.batch_copy_emit(ref, None, case.n, src, copies, case.pl.stride, case.pl.length, case.kind)
                else:
                    rst = oracle.batch_copy_emit(ref, case.desc, case.n, src, copies)
                assert np.array_equal(ref, case.ref(CAPS[0])[1]), "the copy puts the record back: emit's result as ever"
                d = torch.from_numpy(scrambled[name]).cuda()
                status = torch.zeros(case.n, dtype=torch.uint8, device="cuda:0")
                eng.copy_emit(d, case.batch(), d_src, d_copies, status=status)
                lc = eng.last_launch()
                assert (lc["kernel"], lc["variant"]) == ("copy_kernel", variant), lc
                _check_emitted(case, d, CAPS[0], f"copy_emit {variant} {form} fill {name}")
                _same(status.cpu().numpy(), rst, f"copy_emit {variant} {form}: status")
    finally:
        eng.set_variant(-1)


# ---------------------------------------------------------------------------------------------
# The receive-side batched calls
# ---------------------------------------------------------------------------------------------


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
            # (the edge sweep asks for payloads behind the window; here: delivered payloads of every pattern's length,
            # among them rejected records', which are delivered all the same)
            assert sum(1 for s in spans if s) > case.n // 2 and ((vst & E.ST_ACCEPT) == 0)[[bool(s) for s in spans]].sum() > 100
    finally:
        e.set_shape(-1)


def _reply_fields(arena, slots, ent, written, kinds):
    """The ICMP checksum fields of the written reply frames of an expected arena."""
    out = set()
    for i in np.flatnonzero(written):
        o = int(slots["dst_offset"][i]) + (14 if kinds[i] == E.KIND_ETH else 0)
        l4 = o + (20 if arena[o] >> 4 == 4 else 40)
        out.add(int(arena[l4 + 2]) << 8 | int(arena[l4 + 3]))
    return out


@pytest.mark.parametrize("form,shape", RX_FORMS)
def test_verify_echo_reply(eng, sweep, form, shape):
    """The replies' checksums are the classes here: the corpus holds requests steered so that the reply's ICMP sum is
    C0, C1, CFFFE and all zero (ZERO: 0xffff), and its IPv4 header's H0."""
    rng = np.random.default_rng(4)
    e = eng.prod
    e.set_shape(shape)
    try:
        seen = set()
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
            seen |= _reply_fields(arena, slots, ent, (ent["flags"] & E.ECHO_WRITTEN) != 0, case.pl.kinds)
        assert {0x0000, 0x0001, 0xFFFE, 0xFFFF} <= seen  # (the edge sweep asks for requests behind the window)
    finally:
        e.set_shape(-1)


@pytest.mark.parametrize("form,shape", RX_FORMS)
def test_verify_unreach_reply(eng, sweep, form, shape):
    """The error frames' checksums are the classes here: datagrams to a closed port and of an unknown protocol,
    steered so that the error's ICMP sum is C0, C1 and CFFFE and its two IPv4 header sums H0 and IN0."""
    rng = np.random.default_rng(5)
    e = eng.prod
    port_map = E.make_port_map(set(range(1, 6000)) - set(S.CLOSED_PORTS))
    e.set_shape(shape)
    try:
        seen, forms = set(), set()
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
            seen |= _reply_fields(arena, slots, ent, written, case.pl.kinds)
            forms |= set((ent["flags"][written] & E.UNR_PORT).tolist())
        assert {0x0000, 0x0001, 0xFFFE} <= seen and forms == {0, E.UNR_PORT}
    finally:
        e.set_shape(-1)


@pytest.mark.parametrize("form", ["gaps", "packed", "fixed"])
def test_verify_udp_enqueue(eng, sweep, form):
    """One socket per 64 records, bound to the corpus's first UDP port (tests/test_gpu_udp_enqueue_edges.py's
    arrangement): the rejected verify copies take no space, so their followers move and are RESTORED."""
    e = eng.prod
    rng = np.random.default_rng(6)
    port, PRE, M = S.CLOSED_PORTS[0], 0x5A, 70
    for case in _rx_cases(sweep, form):
        pl, n = case.pl, case.n
        vst = case.ref(CAPS[0])[0]
        groups = [(a, min(64, n - a), 0) for a in range(0, n, 64)]
        dgs = [R.udp_datagram(r, int(k), int(f)) for r, k, f in zip(case.recs, pl.kinds, pl.flags)]
        need = [sum(d[1] for d in dgs[a:a + c] if d and d[3] == port) for a, c, _ in groups]
        caps_ = [max(ndd + 700 + int(rng.integers(0, 16)), 1) for ndd in need]
        base = 7 + np.concatenate([[0], np.cumsum(np.array(caps_[:-1], np.int64) + int(rng.integers(0, 3)))])
        socks = E.make_udpsocks(base, np.arange(len(groups)) * (M + 1) + 1, caps_, [c - 300 for c in caps_], 5, M,
                                rng.integers(0, M, len(groups)), 2, port)
        size, msize = int(base[-1]) + caps_[-1] + 29, len(groups) * (M + 1) + 2
        exp = R.expected(case.recs, pl.kinds, pl.flags, groups, socks, vst, size, msize)
        fl = exp["rx"]["flags"]
        enq = (fl & E.URX_ENQUEUED) != 0
        # (the edge sweep: more than 300 enqueued, payloads behind the window.  Here: datagrams of both zeros in the
        # field are enqueued, the wrong neighbours are not, and what follows them is stored again)
        assert exp["written"].all() and enq.sum() > 100 and (fl & E.URX_RESTORED).any() and (fl == E.URX_UDP).sum() > 50
        fields = {int(case.recs[i][d[0] - 2]) << 8 | case.recs[i][d[0] - 1] for i, d in enumerate(dgs) if d and enq[i]}
        assert {0x0000, 0xFFFF, 0x0001, 0xFFFE} <= fields
        dst = torch.full((size,), ARENA_FILL, dtype=torch.uint8, device="cuda:0")
        md = torch.full((msize, 48), PRE, dtype=torch.uint8, device="cuda:0")
        gd = torch.from_numpy(E.make_groups([g[0] for g in groups], [g[1] for g in groups]).view(np.uint8).copy()).cuda()
        st, rx, out = e.verify_udp_enqueue(case.dev("host"), case.batch(), gd, dst, torch.from_numpy(socks.view(np.uint8).copy()).cuda(), md)
        assert e.last_launch()["kernel"] == "udprx_kernel", e.last_launch()
        _same(st.cpu().numpy(), vst, "verify_udp_enqueue status")
        _same(rx.cpu().numpy().reshape(-1).view(E.UDPRX_DTYPE), exp["rx"], "record entries")
        _same(out.cpu().numpy().reshape(-1).view(E.UDPSOCKOUT_DTYPE), exp["outs"], "group entries")
        want_meta = exp["meta"].view(np.uint8).reshape(msize, 48).copy()
        want_meta[~exp["meta_written"]] = PRE
        bad = np.flatnonzero((md.cpu().numpy() != want_meta).any(axis=1))
        assert bad.size == 0, f"metadata entries differ at {bad[:8]}"
        diff = R.check_arena(dst.cpu().numpy(), exp)
        assert diff.size == 0, f"ring bytes differ at {diff[:8]}"


@pytest.mark.parametrize("form", ["tcpgaps", "tcpfixed"])
def test_verify_tcp_assemble(eng, sweep, form):
    """One connection per 64 of the corpus's TCP records.  The records stay as they are (a rewritten sequence number
    would move the sums off their class): each group's window starts at its first segment's sequence number and is
    as long as the ring, so every accepted segment's place is its own distance from there, wherever that is."""
    e = eng.prod
    for case in sweep.cases(form):
        pl, n = case.pl, case.n
        vst = case.ref(CAPS[0])[0]
        groups = [(a, min(64, n - a), 0) for a in range(0, n, 64)]
        starts = []
        for a, c, _ in groups:
            segs = [tcp_assemble_ref.tcp_segment(case.recs[i], int(pl.kinds[i]), int(pl.flags[i])) for i in range(a, a + c)]
            starts.append(next((t[2] for t in segs if t is not None), 0))
        ring = [4096] * len(groups)
        base = 7 + np.arange(len(groups), dtype=np.int64) * (4096 + 3)
        wins = E.make_tcpwins(base, ring, 0, starts, ring)
        size = int(base[-1]) + 4096 + 29
        segs, flows, arena, written = tcp_assemble_ref.expected(case.recs, pl.kinds, pl.flags, groups, wins, (vst & E.ST_ACCEPT) != 0, size)
        copied = (segs["flags"] & tcp_assemble_ref.SEG_COPIED) != 0
        assert written.all() and copied.sum() >= len(groups) - 1 and ((vst & E.ST_ACCEPT) == 0).sum() > 50  # (each group's first accepted segment at least)
        dst = torch.full((size,), ARENA_FILL, dtype=torch.uint8, device="cuda:0")
        gd = torch.from_numpy(E.make_groups([g[0] for g in groups], [g[1] for g in groups]).view(np.uint8).copy()).cuda()
        st, gs, gf = e.verify_tcp_assemble(case.dev("host"), case.batch(), gd, dst, torch.from_numpy(wins.view(np.uint8).copy()).cuda())
        assert e.last_launch()["kernel"] == "tcpasm_kernel", e.last_launch()
        _same(st.cpu().numpy(), vst, "verify_tcp_assemble status")
        _same(gs.cpu().numpy().reshape(-1).view(E.TCPSEG_DTYPE), segs, "segments")
        _same(gf.cpu().numpy().reshape(-1).view(E.TCPFLOW_DTYPE), flows, "flows")
        _same(dst.cpu().numpy(), arena, "rings")


# ---------------------------------------------------------------------------------------------
# 6LoWPAN NHC UDP
# ---------------------------------------------------------------------------------------------

NHC_CAPS = [(0, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 2, 0, 0, 0), (0, 3, 0, 0, 0)]


def _nhc_check(eng, buf, desc_np, batch, n, addrs, caps, variant=-1, shape=-1, blocks=0):
    """tests/test_gpu_nhc.py's check: verify and emit against the oracle, under the forced variant and shape."""
    d_addrs = torch.from_numpy(addrs.reshape(-1).copy()).cuda()
    eng.set_variant(variant)
    eng.set_shape(shape)
    eng.set_max_blocks(blocks)
    try:
        d = torch.from_numpy(buf.copy()).cuda()
        st = eng.nhc_udp_verify(d, batch, d_addrs, caps=caps).cpu().numpy()
        est = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
        eng.nhc_udp_emit(d, batch, d_addrs, caps=caps, status=est)
        got = d.cpu().numpy()
    finally:
        eng.set_variant(-1)
        eng.set_shape(-1)
        eng.set_max_blocks(0)
    kw = {} if desc_np is not None else {"stride": batch.stride, "length": batch.length}
    _same(st, oracle.batch_nhc_udp_verify(buf.copy(), desc_np, n, addrs, caps=caps, **kw), f"nhc verify {variant} {shape} {caps}")
    ref = buf.copy()
    ref_est = oracle.batch_nhc_udp_emit(ref, desc_np, n, addrs, caps=caps, **kw)
    _same(got, ref, f"nhc emit {variant} {shape} {caps}")
    _same(est.cpu().numpy(), ref_est, "nhc emit status")


@pytest.fixture(scope="module")
def nhc():
    recs = Q.build_nhc()
    buf, offs, lens, addrs = Q.nhc_pack(recs)
    return recs, buf, offs, lens, addrs


@pytest.mark.parametrize("caps", NHC_CAPS)
def test_nhc_descriptor_batch(eng, nhc, caps):
    recs, buf, offs, lens, addrs = nhc
    _nhc_check(eng, buf, P.oracle_desc(offs, lens, 0), E.Batch.from_records(offs, lens, 0, "cuda:0"), len(recs), addrs, caps)


def test_nhc_shapes_and_variants(eng, nhc):
    recs, buf, offs, lens, addrs = nhc
    desc, batch = P.oracle_desc(offs, lens, 0), E.Batch.from_records(offs, lens, 0, "cuda:0")
    for variant in eng.avail((0, 1, 2, 3, 4, 5, 6)):
        for shape, blocks in ((variant % 9, 0), ((variant + 4) % 9, 3)):
            _nhc_check(eng, buf, desc, batch, len(recs), addrs, CAPS[0], variant, shape, blocks)


@pytest.mark.parametrize("stride,length", [(128, 128), (385, 385), (1280, 1200), (1500, 1500), (4001, 4001)])
def test_nhc_fixed_stride(eng, stride, length):
    """The packet fills the record: every class in every port mode, inline and elided, at one length."""
    rng = np.random.default_rng(stride)
    recs, addrs, t = [], [], 0
    for rep in range(3):
        for cls in Q.NHC_CLASSES:
            for mode in range(4):
                for elided in (False, True):
                    t += 1
                    pattern = Q.CONTROL if cls == "CTRL" else tuple(Q.PATTERNS)[t % 5]
                    d, a = Q.nhc_record(rng, mode, elided, length - (1 + P.NHC_PORTS_SIZE[mode] + 2), pattern, cls)
                    if rep == 2 and not elided:  # a wrong neighbour of the field
                        fo = 1 + P.NHC_PORTS_SIZE[mode]
                        d = d[:fo] + Q.inc(Q.rd16(d, fo)).to_bytes(2, "big") + d[fo + 2:]
                    recs.append(d), addrs.append(a)
    n = len(recs)
    addrs = np.frombuffer(b"".join(addrs), np.uint8).reshape(n, 32).copy()
    for base in (0, 3):
        buf = rng.integers(0, 256, base + n * stride + 64, dtype=np.uint8)
        for i, r in enumerate(recs):
            buf[base + i * stride: base + i * stride + length] = np.frombuffer(r, np.uint8)
        for variant in eng.avail((-1, 1, 5)):
            _nhc_check(eng, buf[base:].copy(), None, E.Batch.fixed(n, stride, length, 0), n, addrs, CAPS[0], variant)


# ---------------------------------------------------------------------------------------------
# The fragment kernels and the two cut kernels
# ---------------------------------------------------------------------------------------------

from tests import test_frag_cpu as F  # noqa: E402
from tests import cut_ref  # noqa: E402
from tests.test_gpu_fragment import _run as run_fragment_emit  # noqa: E402
from tests.test_gpu_fragments import _device_frag  # noqa: E402
from tests.test_gpu_reassemble import _run as run_reassemble  # noqa: E402

MTUS = (68, 576, 1500)


def _piece_datagrams(mtu, rng):
    """Datagrams of every protocol, class and piece mode at three lengths (an odd one: a last slice of one byte;
    whole slices; an even remainder), each with another pattern; at MTU 1500 the longest datagram, all 0xff."""
    step, out, t = Q.frag_step(mtu), [], 0
    for proto in ("udp", "tcp", "echo"):
        for mode in Q.PIECE_MODES:
            for cls in Q.TARGET:
                for T in (2 * step + 1, 3 * step, 4 * step + 6):
                    t += 1
                    d = Q.frag_datagram(rng, proto, T, mtu, tuple(Q.PATTERNS)[t % 5], cls, mode, ident=t)
                    got, slices = Q.frag_classes(d, mtu)
                    assert got == cls or (proto, mode) == ("echo", "each0"), (proto, mode, cls, T, got)
                    assert mode != "zeros" or set(slices[1:]) == {"zero"}
                    assert mode != "each0" or set(slices[:-1]) == {"mult"}
                    out.append(d)
    if mtu == 1500:
        out.append(Q.frag_datagram(rng, "udp", 65515, mtu, "ff", "C0", "plain", ident=0x7FFF))
        assert len(out[-1]) == 65535
    return out


@pytest.mark.parametrize("eth", [False, True])
@pytest.mark.parametrize("mtu", MTUS)
def test_fragment_groups(eng, mtu, eth):
    """emit_frag and verify_frag (frag_kernel), then verify_reassemble (fragcopy_kernel), over groups whose slices
    are all zero, each a multiple of 0xffff, or steered apart, the group's checksum on both zeros and their
    neighbours; the fragments in shuffled order at random gaps, so their payloads start at odd and even addresses."""
    rng = np.random.default_rng(mtu + eth)
    dgs = _piece_datagrams(mtu, rng)
    off, ref, groups = F.tx_pair(dgs, mtu, eth, shuffle_rng=rng)
    kind = E.KIND_ETH if eth else E.KIND_IP
    got, offs, lens, vst = _device_frag(eng, off, groups, kind, seed=mtu)
    assert {int(o) % 2 for o in offs} == {0, 1}
    for o, ln, want in zip(offs, lens, ref):
        assert got[int(o):int(o) + int(ln)].tobytes() == want  # "emit whole, then fragment"
    assert (vst & E.ST_ACCEPT).all()
    # the neighbours of each group's checksum are rejected: the first fragment of every group holds the L4 field
    io = 14 if eth else 0
    wrong = [bytearray(r) for r in ref]
    for gi, (f, c) in enumerate(groups):
        for r in wrong[f:f + c]:
            if not int.from_bytes(r[io + 6:io + 8], "big") & 0x1FFF:
                fo = io + 20 + {17: 6, 6: 16, 1: 2}[r[io + 9]]
                v = Q.rd16(r, fo)
                r[fo:fo + 2] = (Q.inc(v) if gi % 2 else Q.dec(v)).to_bytes(2, "big")
    buf, offs2, lens2 = P.pack([bytes(r) for r in wrong], gap_rng=np.random.default_rng(mtu + 7))
    batch = E.Batch.from_records(offs2, lens2, kind, "cuda:0")
    gh = E.make_groups([f for f, _ in groups], [c for _, c in groups])
    gd = torch.from_numpy(gh.view(np.uint8).copy()).cuda()
    wst = eng.prod.verify_frag(torch.from_numpy(buf).cuda(), batch, gd).cpu().numpy()
    _same(wst, oracle.batch_verify_frag(buf, P.oracle_desc(offs2, lens2, kind), len(wrong), gh), "verify_frag of the neighbours")
    assert not (wst & E.ST_ACCEPT).any()
    st, dg = run_reassemble(eng.prod, ref, groups, kind=kind, seed=mtu, accept=True)
    assert (dg["copied"] == 1).all() and [int(x) for x in dg["len"]] == [len(x) - 20 for x in dgs]
    run_reassemble(eng.prod, [bytes(r) for r in wrong], groups, kind=kind, seed=mtu + 1, accept=False)


@pytest.mark.parametrize("fill", list(FILLS))
@pytest.mark.parametrize("mtu", MTUS)
def test_fragment_emit(eng, mtu, fill):
    """fragment_emit (fragcut_kernel): the same datagrams whole, each fill in their checksum fields, frames back to
    back; descriptor batches with and without Ethernet, and a fixed stride for all but the longest."""
    rng = np.random.default_rng(mtu)
    dgs = _piece_datagrams(mtu, rng)
    if FILLS[fill] is not None:
        dgs = [d[:10] + bytes([FILLS[fill]]) * 2 + d[12:] for d in dgs]
        dgs = [d[:fo] + bytes([FILLS[fill]]) * 2 + d[fo + 2:] for d in dgs for fo in [20 + {17: 6, 6: 16, 1: 2}[d[9]]]]
    else:
        dgs = [F.emit_whole(d, F.DEFAULT) for d in dgs]
    for eth in (False, True):
        recs = [P.eth(d) for d in dgs] if eth else dgs
        out, _, _ = run_fragment_emit(eng.prod, recs, kind=E.KIND_ETH if eth else E.KIND_IP, mtu=mtu, seed=mtu + eth)
        assert (out["written"] == 1).all() and (out["count"] >= 3).all()
    short = [d for d in dgs if len(d) < 8000]
    run_fragment_emit(eng.prod, short, mtu=mtu, fixed=(max(len(d) for d in short) + 3, 5), seed=mtu)


@pytest.mark.parametrize("mss", [1, 536, 1460])
def test_tcp_segment_emit(eng, mss):
    """tcp_segment_emit (tcpcut_kernel): sends of each pattern behind IPv4 and IPv6 templates whose sequence number
    carries between its halves (0xffffff00), one word of every MSS slice steered so that each frame's checksum is
    C0, C1 or CFFFE; at MSS 1 the slices have no word and the patterns go unsteered."""
    rng = np.random.default_rng(mss)
    e = eng.prod
    sends, chunks, want = [], [], []
    t = 0
    for v6 in (False, True):
        for eth in (False, True):
            kind = E.KIND_ETH if eth else E.KIND_IP
            for cls in Q.TARGET:
                for pattern in Q.PATTERNS:
                    for ln in ((40,) if mss == 1 else (3 * mss, 2 * mss + 7)):
                        t += 1
                        tpl = tcp_segment_ref.template(rng, v6=v6, eth=eth, doff=(5, 8, 15)[t % 3], seq=0xFFFFFF00)
                        io_t = (14 if eth else 0) + (40 if v6 else 20)
                        pay = Q.steer_send(bytearray(Q._fill(pattern, ln, rng)),
                                           lambda p: tcp_segment_ref.frames_of(tpl, kind, 0, p, mss, CAPS[0])[1], mss, cls, io_t)
                        sends.append((tpl, kind, 0, mss, ln)), chunks.append(bytes(pay)), want.append((cls, io_t))
    n = len(sends)
    recs, kinds = [s[0] for s in sends], np.array([s[1] for s in sends], np.uint8)
    flags_a, msss, lens_p = np.zeros(n, np.uint8), np.full(n, mss, np.uint16), np.array([s[4] for s in sends], np.int64)
    # the payload ranges back to back, one byte between two of them: odd and even source addresses
    so = np.cumsum([0] + [len(c) + 1 for c in chunks[:-1]])
    src = np.frombuffer(b"\x5c".join(chunks), np.uint8).copy()
    assert {int(o) % 2 for o in so} == {0, 1}
    for fixed in (None, (117, 5)):
        buf, offs, lens, placed = cut_ref.place_records(recs, kinds, flags_a, fixed, rng) if fixed is None else (None,) * 4
        for k in ((None,) if fixed is None else (E.KIND_IP, E.KIND_ETH)):
            sel = np.arange(n) if k is None else np.flatnonzero(kinds == k)
            if k is not None:
                buf, offs, lens, placed = cut_ref.place_records([recs[i] for i in sel], kinds[sel], flags_a[sel], fixed, rng)
            plans, slots, ref_out, ref_arena = cut_ref.plan_slots(
                len(sel), lambda o, c: E.make_tcpplans(so[sel], lens_p[sel], msss[sel], o, c),
                lambda pl, size: tcp_segment_ref.expected(placed, kinds[sel], flags_a[sel], pl, src, 0, CAPS[0], size), 0, 3, 0)
            batch, d, dv, dst, pd = cut_ref.upload(E, buf, offs, lens, kinds[sel], flags_a[sel], fixed, plans, ref_arena.size)
            ds = torch.from_numpy(src.copy()).cuda()
            out = e.tcp_segment_emit(dv, batch, ds, dst, pd, frame_stride=0, caps=CAPS[0])
            got_out, _ = cut_ref.compare(e, "tcpcut_kernel", out, dst, ref_out, ref_arena,
                                         [(d, buf, "the batch buffer"), (ds, src, "the payload source")])
            assert (got_out["written"] == 1).all()
            if mss > 1:  # every frame's checksum is its send's class, in the reference arena the device equals
                for j, i in enumerate(sel):
                    cls, io_t = want[i]
                    o, fl = int(slots[j]), int(ref_out[j]["frame_len"])
                    for f in range(int(ref_out[j]["count"])):
                        at = o + f * fl + io_t + 16
                        assert ref_arena[at:at + 2].tobytes() == Q.TARGET[cls].to_bytes(2, "big"), (i, f, cls)
