"""verify_udp_enqueue with 64-bit byte offsets at and past 4 GiB, on the sparse-arena rig of tests/far.py: the
sockets' frames NEAR, across and past 2^32, their payload rings NEAR, across and past it with a payload range
across it, their metadata rings on both sides of it (tests/far_udp_enqueue.py).  Status bytes, record and group
entries equal tests/udp_enqueue_ref.py's; both arenas are scanned for strays, the metadata entries included.
The module skips only when the device has less than 12 GiB free."""
import numpy as np
import pytest

from tests import far_udp_enqueue as FU

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from smoltcp_amd import engine as E  # noqa: E402
from tests.test_gpu_far_offsets import SEAM, SIZE, _dev, _pre, rig  # noqa: E402,F401  (rig: this module's own)


@pytest.mark.parametrize("rot", [0, 1, 2])
def test_udp_enqueue_rings_across_the_seam(rig, rot):  # noqa: F811
    """FU.udprx_case; d_meta is the rings' arena itself, so meta_first * 48 passes 2^32 for two sockets."""
    eng = rig.eng.prod
    c = FU.udprx_case(SEAM, SIZE, rot)
    case, n = c.case, c.case.n
    case.fill(rig.a)
    rig.b.refill()
    assert rig.b.buf.data_ptr() % 16 == 0
    st, rx, out = eng.verify_udp_enqueue(rig.a.buf, case.batch_of(), _dev(c.groups), rig.b.buf, _dev(c.socks), rig.b.buf,
                                         status=_pre(n), rx=_pre(n, 16), out=_pre(4, 32))
    launched = eng.last_launch()
    assert launched["kernel"] == "udprx_kernel" and launched["G"] == 64, launched
    assert np.array_equal(st.cpu().numpy(), c.ref_st)
    got_rx = rx.cpu().numpy().reshape(-1).view(E.UDPRX_DTYPE)
    bad = np.flatnonzero(got_rx != c.exp["rx"])
    assert bad.size == 0, (bad[:8], got_rx[bad[:4]], c.exp["rx"][bad[:4]])
    got_out = out.cpu().numpy().reshape(-1).view(E.UDPSOCKOUT_DTYPE)
    assert np.array_equal(got_out, c.exp["outs"]), (got_out, c.exp["outs"])
    rig.b.check(FU.ring_extents(c, rig.b.get) + c.meta_ext)
    rig.a.check(case.place.expected(case.compact))
    print(f"far verify_udp_enqueue rot {rot}: {launched['kernel']}, rings {c.ring_of}, restored {got_out['restored'].tolist()}")
