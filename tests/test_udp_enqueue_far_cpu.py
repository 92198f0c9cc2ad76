"""tests/far_udp_enqueue.py's builder on the host, at the small seam of tests/test_far_rig_cpu.py: its own
conditions hold (enough STRADDLE and FAR frames delivered, every placement pair, a payload range across the
seam, metadata rings on both sides of it), the sparse layouts replay to the compact ones, and the model over the
frames read back from their far places equals the model over the compact buffer."""
import numpy as np
import pytest

from smoltcp_amd import engine as E
from tests import far as F
from tests import far_udp_enqueue as FU
from tests import udp_enqueue_ref as R
from tests.test_far_rig_cpu import SEAM, SIZE, _arena, _replay


@pytest.mark.parametrize("rot", [0, 1, 2])
def test_udp_enqueue_builder(rot):
    c = FU.udprx_case(SEAM, SIZE, rot)
    case = c.case
    lo = int(c.socks["dst_offset"][c.ring_of.index(0)])
    assert lo < SEAM < lo + FU.RL and lo + FU.CUT == SEAM
    assert (F.STRADDLE, (F.STRADDLE, F.NEAR, F.FAR_LO)[c.ring_of[0]]) in c.pairs
    mf = c.socks["meta_first"].astype(np.int64) * 48
    assert (mf >= SEAM).sum() == 2 and (mf + 48 * FU.M < SEAM).sum() == 2
    # with the model's own arena standing in for the device's, the rings' extents are the accepted layout's
    rings = FU.ring_extents(c, lambda a, z: np.full(z - a, c.fill, np.uint8))
    _replay(case, case.compact, rings + c.meta_ext)
    # the frames read back from their far places give the same entries
    arena = _arena()
    case.fill(arena)
    far_offs = case.desc_far["offset"].astype(np.int64)
    placed = [bytes(arena.get(int(o), int(o) + int(ln))) for o, ln in zip(far_offs, case.lens)]
    g = [(int(a), int(b), 0) for a, b in zip(c.groups["first"], c.groups["count"])]
    compact = c.socks.copy()
    compact["dst_offset"] = [3 + k * (FU.RL + 11) for k in range(4)]
    compact["meta_first"] = [1 + k * (FU.M + 1) for k in range(4)]
    again = R.expected(placed, case.kinds, np.zeros(case.n, np.uint8), g, compact, c.ref_st, c.exp["arena"].size, c.exp["meta"].size)
    for key in ("rx", "outs", "arena", "meta", "spec_only"):
        assert np.array_equal(again[key], c.exp[key]), key
    # a speculative byte left in free space passes the rings' check, any third value there does not
    only = np.flatnonzero(c.exp["spec_only"])
    assert only.size > 0
    dev = c.exp["arena"].copy()
    dev[only[0]] = c.exp["spec_arena"][only[0]]
    second = _arena()
    ext0 = [(f, dev[a:b]) for a, b, f in c.dplace.ext]
    for f, b in ext0:
        second.put(f, b)
    second.check(FU.ring_extents(c, second.get))
    if c.exp["spec_arena"][only[0]] != c.fill ^ 0xFF:
        second.put(int(c.dplace.far(only[0])), bytes([c.fill ^ 0xFF]))
        with pytest.raises(AssertionError):
            second.check(FU.ring_extents(c, second.get))
