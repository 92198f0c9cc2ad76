"""The edge sweep's corpus on the CPU (tests/edge_sweep.py): every cell of every window model is hit in
every placement form, the oracle, the Python model over oracle/pyref.py and the C++ host mirror's scalar
sums agree on the whole corpus, and the coverage assertion fails when the odd start addresses are left
out.  The GPU side is tests/test_gpu_edge_sweep.py."""
import os
import subprocess

import numpy as np
import pytest

import oracle
from oracle import pyref
from smoltcp_amd import engine as E
from tests import edge_sweep as S
from tests import pktgen as P

CAPS = [(0, 0, 0, 0, 0), (2, 3, 0, 1, 0)]
FORMS = ("packed", "gaps", "fixed")

# The cells geometry cannot reach.  A cell is (object, x) with x = head + record offset and head < grid,
# so x is at most grid - 1 + the object's largest record offset.  Ethernet adds 14 and an IPv4 header at
# most 60 bytes:
#   IPv4 header checksum      14 + 10          = 24
#   IPv4 header's last byte   14 + 60 - 1      = 73
#   ICMPv4 / IGMP checksum    14 + 60 + 2      = 76   (both ride IPv4 only)
#   embedded header checksum  14 + 60 + 8 + 10 = 92
#   embedded header last byte 14 + 60 + 8 + 59 = 141
# 96 B on the 16-B grid:   x <= 15 + 24 = 39, 15 + 73 = 88, 15 + 76 = 91 stay below 94 (95 for a last byte);
#                          15 + 92 = 107 and 15 + 141 = 156 reach 96 and 97.
# 128 B on the 16-B grid:  107 stays below 126 as well; 156 reaches 129.
# 256 B on the 128-B grid: x <= 127 + 24 = 151, 127 + 73 = 200, 127 + 76 = 203, 127 + 92 = 219 stay below 254;
#                          127 + 141 = 268 reaches 257.
# Every object IPv6 carries behind a Hop-by-Hop header (up to 2048 B) reaches every x.
UNREACHABLE = {
    (96, 16): [("ipck", (94, 95, 96)), ("iplast", (95, 96, 97)), ("l4ck_icmp4", (94, 95, 96)), ("l4ck_igmp", (94, 95, 96))],
    (128, 16): [("ipck", (126, 127, 128)), ("iplast", (127, 128, 129)), ("l4ck_icmp4", (126, 127, 128)),
                ("l4ck_igmp", (126, 127, 128)), ("inck", (126, 127, 128))],
    (256, 128): [("ipck", (254, 255, 256)), ("iplast", (255, 256, 257)), ("l4ck_icmp4", (254, 255, 256)),
                 ("l4ck_igmp", (254, 255, 256)), ("inck", (254, 255, 256))],
}


def _unreachable(model):
    return {S.window_cell(model, c, x) for c, xs in UNREACHABLE[model] for x in xs}


@pytest.fixture(scope="module")
def corpus():
    return S.build_corpus()


def _place(corpus, form, keep=lambda res: True):
    if form == "fixed":
        return [S.place_fixed(corpus, k, f, keep=keep) for k in (S.KIND_IP, S.KIND_ETH) for f in (0, S.REC_IPHDR_ONLY)]
    return [S.place_desc(corpus, gaps=form == "gaps", keep=keep)]


def _assert_covered(placed, model):
    good, bad = S.coverage(placed, model)
    want = S.all_cells(model) - _unreachable(model)
    assert not want - good, f"no record hits {sorted(want - good)[:12]}"
    assert not good & _unreachable(model), sorted(good & _unreachable(model))
    # a record cut short of its IP length is MALFORMED: no bad checksum changes its verdict
    want_bad = {c for c in want if not c.startswith("spanend:cut")}
    assert not want_bad - bad, f"no bad-checksum copy hits {sorted(want_bad - bad)[:12]}"


def test_the_listed_cells_are_the_arithmetic():
    for model in S.MODELS:
        assert _unreachable(model) == S.unreachable_cells(model)
        assert len(S.all_cells(model)) == 168


def test_corpus_size(corpus):
    assert 8000 <= len(corpus) <= 25000
    assert max(len(r.data) for r in corpus) == S.LMAX
    nbad = sum(r.bad is not None for r in corpus)
    assert nbad * 7 >= len(corpus)  # one in five of the untouched records, and more where a cell asked for one
    assert {r.bad for r in corpus} == {None, "field0", "field1", "last", "after"}
    assert {(r.kind, r.flags) for r in corpus} == {(k, f) for k in (1, 2) for f in (0, 1)}
    hbh = [S.geometry(r.data, r.kind, r.flags).l4_off for r in corpus if r.family == "v6/hbh"]
    for edge in (96, 128, 256, 1024, 2048):  # the L4 header walks over each
        assert {edge - 8 <= o < edge for o in hbh} == {True, False} and any(edge <= o < edge + 8 for o in hbh)


@pytest.mark.parametrize("form", FORMS)
def test_every_cell_is_hit(corpus, form):
    placed = _place(corpus, form)
    for pl in placed:
        assert pl.buf.size < 64 << 20
        starts = pl.offs[pl.index >= 0] % 128
        assert np.array_equal(starts, [corpus[i].res for i in pl.index[pl.index >= 0]])
        used = np.zeros(pl.buf.size, bool)
        for o, n in zip(pl.offs, pl.lens):
            assert not used[int(o):int(o + n)].any()
            used[int(o):int(o + n)] = True
        assert (pl.buf[~used] == S.SENTINEL).all()
        if form == "packed":
            assert np.array_equal(pl.offs[1:], (pl.offs + pl.lens)[:-1])
        if form == "fixed":
            assert pl.stride % 2 == 1 and set((pl.offs % 128).tolist()) == set(range(128))
    assert sorted(i for pl in placed for i in pl.index if i >= 0) == list(range(len(corpus)))
    for model in S.MODELS:
        _assert_covered(placed, model)


@pytest.mark.parametrize("length", [2304, 4032])
def test_the_transposed_walk_lengths_keep_every_cell(corpus, length):
    """Padded to 2304 / 4032 B the layouts stay under 64 MiB (thinned where a start residue holds more
    records than slots) and lose none of the header cells; the span-end cells belong to the other forms."""
    placed = [S.place_fixed(corpus, k, 0, length, length + 1) for k in (S.KIND_IP, S.KIND_ETH)]
    assert all(pl.buf.size < 64 << 20 for pl in placed)
    for model in S.MODELS:
        good, bad = S.coverage(placed, model)
        want = {c for c in S.all_cells(model) - _unreachable(model) if not c.startswith("span")}
        assert not want - good and not want - bad, sorted((want - good) | (want - bad))[:12]


@pytest.mark.parametrize("form", FORMS)
def test_without_the_odd_starts_the_coverage_fails(corpus, form):
    placed = _place(corpus, form, keep=lambda res: res % 2 == 0)
    for model in S.MODELS:
        with pytest.raises(AssertionError, match="no record hits"):
            _assert_covered(placed, model)
        good, _ = S.coverage(placed, model)
        lost = S.all_cells(model) - _unreachable(model) - good
        W = model[0]
        assert S.window_cell(model, "l4ck_udp", W - 1) in lost  # an even field offset needs an odd start here


@pytest.mark.parametrize("caps", CAPS)
def test_oracle_and_model_agree(corpus, caps):
    """Status, emitted bytes and field entries over the whole corpus: oracle/csum_oracle.c against the
    Python model over oracle/pyref.py."""
    recs = [r.data for r in corpus]
    kinds = np.array([r.kind for r in corpus], np.uint8)
    flags = np.array([r.flags for r in corpus], np.uint8)
    buf, offs, lens = P.pack(recs)
    desc = P.oracle_desc(offs, lens, kinds, flags)
    st = oracle.batch_verify(buf, desc, len(desc), caps=caps)
    model_st = np.array([S.verify_model(r.data, r.kind, r.flags, caps) for r in corpus], np.uint8)
    bad = np.flatnonzero(st != model_st)
    assert bad.size == 0, (bad[:8], st[bad[:8]], model_st[bad[:8]])
    if caps == CAPS[0]:
        untouched = np.array([r.bad is None for r in corpus])
        gate = (st & (S.ST_MALFORMED | S.ST_UNSUPPORTED)) == 0
        assert (st[untouched & gate] & S.ST_ACCEPT).all()
        for i, r in enumerate(corpus):
            if r.bad == "after":  # the first byte after the span: the verdict stays
                assert st[i] == st[r.twin], i
        assert sum(not st[i] & S.ST_ACCEPT for i, r in enumerate(corpus) if r.bad in ("field0", "field1", "last")) > 1000
    # emit over 0xA5A5 in every checksum field
    raw = buf.copy()
    for r, o in zip(corpus, offs):
        for f in S.field_offsets(r.data, r.kind, r.flags):
            if f is not None:
                raw[int(o) + f:int(o) + f + 2] = 0xA5
    ref = raw.copy()
    est = oracle.batch_emit(ref, desc, len(desc), caps=caps)
    entries = np.zeros(len(corpus), E.FIELDS_DTYPE)
    for i, (r, o, n) in enumerate(zip(corpus, offs, lens)):
        rec = bytearray(raw[int(o):int(o + n)].tobytes())
        s, ent = S.emit_model(rec, r.kind, r.flags, caps)
        assert s == est[i], i
        assert bytes(rec) == ref[int(o):int(o + n)].tobytes(), (i, r.family)
        entries[i]["off"], entries[i]["val"], entries[i]["status"] = [e[0] for e in ent], [e[1] for e in ent], s
    patched = raw.copy()
    assert E.apply_fields(patched, offs.astype(np.int64), lens.astype(np.int64), entries).all()
    assert np.array_equal(patched, ref)
    if caps == CAPS[0]:
        ok = np.array([r.bad is None for r in corpus])  # (emit repairs a bad copy's field)
        for i in np.flatnonzero(ok):
            o, n = int(offs[i]), int(lens[i])
            assert np.array_equal(ref[o:o + n], buf[o:o + n]), i  # emit puts back what the corpus holds


def test_host_mirror_sums_the_corpus_spans(corpus, tmp_path):
    """The C++ host mirror (smoltcp_amd/host/smoltcp_checksum.hpp) through tests/cpp/test_host_mirror's
    vector mode: checksum::data over every summed L4 span of the corpus."""
    cpp = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")
    import fcntl

    with open(os.path.join(cpp, ".make.lock"), "w") as lk:  # one make at a time (tests/test_host_cpp.py)
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.run(["make", "-s", "-C", cpp], check=True)
    lines = []
    for r in corpus:
        g = S.geometry(r.data, r.kind, r.flags)
        if g.gate:
            span = r.data[g.l4_off:S.span_end(r.data, g)]
            lines.append(f"data {span.hex() or '-'} {pyref.data(span)}")
    p = tmp_path / "vectors.txt"
    p.write_text("\n".join(lines) + "\n")
    out = subprocess.run([os.path.join(cpp, "test_host_mirror"), "vectors", str(p)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert f"vectors {len(lines)}" in out.stdout and len(lines) > 3000


def _emit_with_a_fault(pl, model):
    """(the oracle's emit of a placed corpus, a stand-in's): the stand-in is a kernel whose byte-wise field
    store loses the byte behind its window, so a checksum field whose first byte is the window's last byte
    goes out half."""
    W, grid = model
    raw = pl.buf.copy()
    hit = []
    for i in range(pl.n):
        o = int(pl.offs[i])
        for f in S.field_offsets(pl.record(i), int(pl.kinds[i]), int(pl.flags[i])):
            if f is not None:
                raw[o + f:o + f + 2] = 0xA5
                if o % grid + f == W - 1:
                    hit.append(o + f + 1)
    ref = raw.copy()
    oracle.batch_emit(ref, P.oracle_desc(pl.offs, pl.lens, pl.kinds, pl.flags), pl.n)
    got = ref.copy()
    got[hit] = raw[hit]
    return ref, got


@pytest.mark.parametrize("model", S.MODELS)
def test_a_kernel_wrong_in_one_cell_is_noticed(corpus, model):
    """The GPU module's comparison (the whole emitted buffer) sees a kernel that is wrong in the one cell
    'field at W - 1' of one window model, and would not without the odd start addresses: every checksum
    field sits at an even record offset, so W - 1 - offset is odd."""
    ref, got = _emit_with_a_fault(S.place_desc(corpus, gaps=True), model)
    assert (ref != got).sum() >= 2
    ref, got = _emit_with_a_fault(S.place_desc(corpus, gaps=True, keep=lambda res: res % 2 == 0), model)
    assert np.array_equal(ref, got)
