"""Every transposed-walk variant of the registry (smoltcp_amd/csrc/variants.def), forced, against the
CPU oracle: the rows no other oracle test forces are the ones a mis-wired row would hide in."""
import ctypes

import numpy as np
import pytest

import oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from smoltcp_amd import _lib  # noqa: E402
from smoltcp_amd import engine as E  # noqa: E402
from tests.engines import VariantEngine  # noqa: E402

CAPS = (0, 0, 0, 0, 0)
F_XWALK, V_NOSTORE = 2, 32


def _xwalk_variants():
    """The registry's xwalk rows whose forms store (a no-store form writes wrong bytes by design)."""
    L, info, out = _lib.lib(), (ctypes.c_int * 4)(), []
    for v in range(128):
        if L.smol_csum_tool_variant_info(v, info) == 0 and info[0] == F_XWALK and not info[1] & V_NOSTORE:
            out.append(v)
    return out


def test_every_xwalk_variant_against_the_oracle():
    """Emit (the whole buffer) and verify (the status bytes, after corrupt(every=7)) of every storing
    transposed-walk variant, forced, equal the oracle's, and last_launch names xwalk_kernel and the
    variant.  One length per records-per-wavefront count (1500: 8, 1922: 4, 3970: 2, 8066: 1); 1, 9 and
    65 records: a partial wavefront, a second wavefront, a second workgroup (also of the 64-record
    workgroups of 107 and 113); packed and with a 1-byte gap; IPv4/UDP and the IPv6 mix.  The oracle's
    answers are computed once per batch and shared by the variants."""
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    eng = VariantEngine(0)
    try:
        variants = eng.avail(_xwalk_variants())
        assert {43, 44, 47, 57, 58, 80, 82, 88, 89, 90, 93, 99, 101, 107, 108, 110, 112, 113} <= set(variants)
        for length in (1500, 1922, 3970, 8066):
            for n in (1, 9, 65):
                for gap in (0, 1):
                    for profile in (E.SYNTH_UDP4, E.SYNTH_V6MIX):
                        stride = length + gap
                        batch = E.Batch.fixed(n, stride, length, E.KIND_IP)
                        raw = torch.zeros(n * stride + 64, dtype=torch.uint8, device="cuda:0")
                        eng.synth(raw, batch, profile, seed=1000 * length + 10 * n + gap)
                        want_e = raw.cpu().numpy().copy()
                        oracle.batch_emit(want_e, None, n, stride, length, E.KIND_IP, CAPS)
                        bad = torch.from_numpy(want_e).to("cuda:0")
                        eng.corrupt(bad, batch, every=7, seed=7)
                        want_v = oracle.batch_verify(bad.cpu().numpy(), None, n, stride, length, E.KIND_IP, CAPS)
                        want_e, want_v = torch.from_numpy(want_e).to("cuda:0"), torch.from_numpy(want_v).to("cuda:0")
                        for v in variants:
                            case = (v, length, n, gap, profile)
                            got = raw.clone()
                            eng.set_variant(v)
                            try:
                                eng.emit(got, batch)
                                le = eng.last_launch()
                                st = eng.verify(bad, batch)
                                lv = eng.last_launch()
                            finally:
                                eng.set_variant(-1)
                            assert (le["kernel"], le["variant"]) == ("xwalk_kernel", v), (case, le)
                            assert (lv["kernel"], lv["variant"]) == ("xwalk_kernel", v), (case, lv)
                            assert torch.equal(got, want_e), case
                            assert torch.equal(st, want_v), case
    finally:
        eng.close()
