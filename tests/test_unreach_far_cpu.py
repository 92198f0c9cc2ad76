"""tests/far_unreach.py's builder on the host, at the small seam of tests/test_far_rig_cpu.py: its own
conditions hold (enough STRADDLE and FAR objects written, every placement pair), the sparse layout replays to
the compact one, and an engine that drops the high word of the port map's address would show."""
import numpy as np
import pytest

from smoltcp_amd import engine as E
from tests import far as F
from tests import far_unreach as FU
from tests import unreach_ref as R
from tests.test_far_rig_cpu import SEAM, SIZE, _arena


@pytest.mark.parametrize("seam_at", ["inside", "end", "far-inside"])
@pytest.mark.parametrize("kind", [E.KIND_IP, E.KIND_ETH])
def test_unreach_reply_builder(kind, seam_at):
    c = FU.unreach_case(SEAM, SIZE, kind, seam_at)
    case = c.case
    assert F.BASE_PAIRS <= c.pairs
    # the records and the port map in a sparse arena: the reference over the records read back from their far
    # places equals the reference over the compact buffer
    arena = _arena()
    case.fill(arena)
    arena.put(c.map_far, c.ports)
    far_offs = case.desc_far["offset"].astype(np.int64)
    placed = [bytes(arena.get(int(o), int(o) + int(ln))) for o, ln in zip(far_offs, case.lens)]
    need = c.slots["cap"].astype(np.int64)
    compact = np.concatenate([[0], np.cumsum(need)[:-1]])
    pm = arena.get(c.map_far, c.map_far + 8192)
    st, ent, _ = R.expected(placed, case.kinds, 0, F.NOCAPS, None, pm, E.make_slots(compact, need), int(need.sum()) + 16)
    assert np.array_equal(st, c.ref_st) and np.array_equal(ent, c.ref_ent)
    arena.check(case.place.expected(case.compact) + [(c.map_far, c.ports)])
    # the map lies past the seam, and what lies at its address with the high word dropped is the arena's fill:
    # every port would read as open there (0xA5 has bits set and clear: port 4000's bit is set), nothing refused
    assert c.map_far >= SEAM
    low = arena.get(c.map_far - SEAM, c.map_far - SEAM + 8192)
    assert (low == F.DST_FILL).all() and R.port_open(low, FU.CLOSED)
    _, ent_low, _ = R.expected(placed, case.kinds, 0, F.NOCAPS, None, low, E.make_slots(compact, need), int(need.sum()) + 16)
    assert not np.array_equal(ent_low, c.ref_ent)
