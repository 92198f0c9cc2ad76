"""verify_udp_enqueue over the edge sweep's corpus (tests/edge_sweep.py): every header object the kernel reads
through its 128-byte window (the UDP ports, the length field, the addresses, the Hop-by-Hop header in front of
them) at every edge of the window and of the 16-byte chunks, in the sweep's three layouts.  The corpus, its
placements and the oracle's references are the sweep's own (tests/test_gpu_edge_sweep.py's Sweep and Case,
imported); the expected entries, metadata and ring bytes are tests/udp_enqueue_ref.py's.

One socket per 64 records, bound to the corpus's first UDP port: its datagrams are candidates, those to the
second port a mismatch, everything else no candidate.  The corpus's bad-checksum copies take no space, so their
followers move and are RESTORED."""
import numpy as np
import pytest

from tests import edge_sweep as S
from tests import udp_enqueue_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from smoltcp_amd import engine as E  # noqa: E402
from tests.test_gpu_edge_sweep import ARENA_FILL, CAPS, _rx_cases, _same, eng, sweep  # noqa: E402,F401  (fixtures: this module's own)

PRE = 0x5A
assert ARENA_FILL == R.SENTINEL


@pytest.mark.parametrize("form", ["gaps", "packed", "fixed"])
def test_verify_udp_enqueue(eng, sweep, form):  # noqa: F811
    e = eng.prod
    rng = np.random.default_rng(6)
    port = S.CLOSED_PORTS[0]
    for case in _rx_cases(sweep, form):
        pl, n = case.pl, case.n
        vst = case.ref(CAPS[0])[0]
        groups = [(a, min(64, n - a), 0) for a in range(0, n, 64)]
        dgs = [R.udp_datagram(r, int(k), int(f)) for r, k, f in zip(case.recs, pl.kinds, pl.flags)]
        # each ring holds its group's candidates and wraps once on the way: it starts 300 bytes before its end
        need = [sum(d[1] for d in dgs[a:a + c] if d and d[3] == port) for a, c, _ in groups]
        caps_ = [max(ndd + 700 + int(rng.integers(0, 16)), 1) for ndd in need]
        base = 7 + np.concatenate([[0], np.cumsum(np.array(caps_[:-1], np.int64) + int(rng.integers(0, 3)))])
        M = 70
        socks = E.make_udpsocks(base, np.arange(len(groups)) * (M + 1) + 1, caps_, [c - 300 for c in caps_], 5, M,
                                rng.integers(0, M, len(groups)), 2, port)
        size, msize = int(base[-1]) + caps_[-1] + 29, len(groups) * (M + 1) + 2
        exp = R.expected(case.recs, pl.kinds, pl.flags, groups, socks, vst, size, msize)
        fl = exp["rx"]["flags"]
        enq = (fl & E.URX_ENQUEUED) != 0
        assert exp["written"].all() and enq.sum() > 300 and (fl & E.URX_RESTORED).any() and (fl == E.URX_UDP).any()
        assert not (fl & E.URX_FULL).any() and (fl & E.URX_PADDED).any()
        assert (exp["rx"]["off"][enq] > 128).sum() > 20  # payloads (and UDP headers) behind the 128-B window
        assert sum(1 for d in dgs if d and d[3] != port) > 20  # the port mismatch
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
        got = dst.cpu().numpy()
        diff = R.check_arena(got, exp)
        assert diff.size == 0, f"ring bytes differ at {diff[:8]} (got {got[diff[:8]]} want {exp['arena'][diff[:8]]})"
