"""verify_unreach_reply with 64-bit byte offsets at and past 4 GiB, on the sparse-arena rig of tests/far.py:
refused datagrams NEAR, across and past 2^32, the port map past it, the error frames' slots back to back across
it (tests/far_unreach.py).  Status bytes, entries and the frames' arena equal tests/unreach_ref.py's; both arenas
are scanned for strays.  The module skips only when the device has less than 12 GiB free."""
import numpy as np
import pytest

from tests import far as F
from tests import far_unreach as FU

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from smoltcp_amd import engine as E  # noqa: E402
from tests.test_gpu_far_offsets import SEAM, SIZE, _dev, _pre, rig  # noqa: E402,F401  (rig: this module's own)
from tests.test_gpu_unreach_reply import SHAPES  # noqa: E402


@pytest.mark.parametrize("seam_at", ["inside", "end", "far-inside"])
@pytest.mark.parametrize("kind", [E.KIND_IP, E.KIND_ETH])
def test_unreach_reply_slots_across_the_seam(rig, kind, seam_at):  # noqa: F811
    """FU.unreach_case; every launch shape of the kernel's shape set."""
    eng = rig.eng.prod
    c = FU.unreach_case(SEAM, SIZE, kind, seam_at)
    case, n, slots = c.case, c.case.n, _dev(c.slots)
    case.fill(rig.a)
    rig.a.put(c.map_far, c.ports)
    pmap = rig.a.buf[c.map_far:c.map_far + 8192]
    for shape in sorted(SHAPES):
        rig.b.refill()
        eng.set_shape(shape)
        try:
            st, ent = eng.verify_unreach_reply(rig.a.buf, case.batch_of(), rig.b.buf, slots, pmap, status=_pre(n), unr=_pre(n, 8))
            launched = eng.last_launch()
        finally:
            eng.set_shape(-1)
        assert launched["kernel"] == "unreach" and launched["variant"] == 0, launched
        assert (launched["G"], launched["U"]) == SHAPES[shape], launched
        got_st, got_ent = st.cpu().numpy(), ent.cpu().numpy().reshape(-1).view(E.UNR_DTYPE)
        assert np.array_equal(got_st, c.ref_st), (shape, np.flatnonzero(got_st != c.ref_st)[:8])
        bad = np.flatnonzero(got_ent != c.ref_ent)
        assert bad.size == 0, (shape, bad[:8], got_ent[bad[:4]], c.ref_ent[bad[:4]], case.where[bad[:4]], c.dwhere[bad[:4]])
        try:
            rig.b.check(c.dplace.expected(c.ref_arena))
        except AssertionError as e:
            raise AssertionError(f"shape {shape}: {e}") from None
    rig.a.check(case.place.expected(case.compact) + [(c.map_far, c.ports)])
    print(f"far verify_unreach_reply kind {kind} {seam_at}: unreach, shapes {sorted(SHAPES)}")
