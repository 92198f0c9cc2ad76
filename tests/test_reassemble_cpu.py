"""CPU-side checks of verify_reassemble (smol_csum_batch_verify_reassemble): the symbol, the datagram
struct in its three spellings (header, ctypes, numpy), the argument errors that need no device, and
tests/reassemble_ref.py, the numpy restatement of the reassembly that the GPU tests
(tests/test_gpu_reassemble.py) take their expected datagram entries and destination bytes from.  No kernel
is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest

import smoltcp_amd
from smoltcp_amd import _lib
from smoltcp_amd import engine as E
from tests import pktgen as P
from tests import reassemble_ref as R
from tests import test_frag_cpu as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "smol_csum_batch_verify_reassemble"


def test_symbol_declared_exported_and_listed():
    with open(os.path.join(ROOT, "include", "smolcsum.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    L = smoltcp_amd.lib()
    assert re.search(r"\b%s\s*\(" % NAME, text)
    assert hasattr(L, NAME) and NAME in _lib.ABI_SYMBOLS
    assert "smol_csum_dgram_t" in text
    assert L.smol_csum_abi_version() == 6  # additive: the version stays


def test_dgram_struct_is_16_bytes_in_every_spelling():
    assert ctypes.sizeof(_lib.DgramC) == 16 == E.DGRAM_DTYPE.itemsize == R.DGRAM_DTYPE.itemsize
    assert E.DGRAM_DTYPE == R.DGRAM_DTYPE
    d = _lib.DgramC(0x04030201, 0x08070605, 0x0A09, 11, 12, 0x100F0E0D)
    assert list(bytes(d)) == list(range(1, 17))
    a = np.frombuffer(bytes(d), dtype=E.DGRAM_DTYPE)[0]
    assert (int(a["len"]), int(a["l4_len"]), int(a["l4_off"]), int(a["protocol"]), int(a["copied"]), int(a["reserved"])) == \
        (0x04030201, 0x08070605, 0x0A09, 11, 12, 0x100F0E0D)


def test_argument_errors_need_no_device():
    L = smoltcp_amd.lib()
    b = _lib.BatchC()
    b.n, b.stride, b.len, b.kind = 4, 64, 64, 1
    caps = _lib.Caps()
    buf = (ctypes.c_uint8 * 256)()
    dst = (ctypes.c_uint8 * 64)()
    st = (ctypes.c_uint8 * 8)()
    raw = (ctypes.c_uint8 * 80)()
    al = (ctypes.addressof(raw) + 15) & ~15  # 16-byte aligned: groups at al, slots at al + 16, dgrams at al + 32
    g, s, d = al, al + 16, al + 32
    ctx = ctypes.c_void_p(1)  # never dereferenced: every case below fails its argument checks first
    call = getattr(L, NAME)
    B, C = ctypes.byref(b), ctypes.byref(caps)
    EINVAL = _lib.SMOL_EINVAL
    assert call(None, buf, B, g, 1, C, dst, s, st, d, None) == EINVAL  # NULL ctx
    assert call(None, buf, B, g, 0, C, dst, s, st, d, None) == EINVAL  # NULL ctx, also with nothing to do
    assert call(ctx, buf, B, g, 1, None, dst, s, st, d, None) == EINVAL  # NULL caps
    assert call(ctx, buf, B, None, 1, C, dst, s, st, d, None) == EINVAL  # NULL d_groups
    assert call(ctx, buf, B, g, 1, C, None, s, st, d, None) == EINVAL  # NULL d_dst
    assert call(ctx, buf, B, g, 1, C, dst, None, st, d, None) == EINVAL  # NULL d_slots
    assert call(ctx, buf, B, g, 1, C, dst, s, None, d, None) == EINVAL  # NULL d_status
    assert call(ctx, buf, B, g, 1, C, dst, s, st, None, None) == EINVAL  # NULL d_dgrams
    assert call(ctx, buf, B, g, 1, C, dst, s + 8, st, d, None) == EINVAL  # d_slots not 16-byte aligned
    assert call(ctx, buf, B, g, 1, C, dst, s, st, d + 4, None) == EINVAL  # d_dgrams not 16-byte aligned
    bad = _lib.Caps()
    bad.udp = 4
    assert call(ctx, buf, B, g, 1, ctypes.byref(bad), dst, s, st, d, None) == EINVAL  # bad caps value
    b.len = (1 << 30) + 1  # past SMOL_MAX_RECORD_LEN, as verify_frag
    assert call(ctx, buf, B, g, 1, C, dst, s, st, d, None) == _lib.SMOL_ERANGE
    assert L.smol_csum_batch_verify_frag(ctx, buf, B, g, 1, C, st, None) == _lib.SMOL_ERANGE
    b.len = 64  # no groups: OK whatever the arrays are, nothing launched
    assert call(ctx, buf, B, None, 0, C, None, None, None, None, None) == _lib.SMOL_OK


def _expected_one_group(recs, kind, flags=0, cap=None):
    n = len(recs)
    T = sum(len(r) for r in recs)  # an upper bound of any payload
    dg, arena = R.expected(recs, [kind] * n, [flags] * n, [(0, n, 0)], [3], [T if cap is None else cap], T + 8)
    return dg[0], arena


@pytest.mark.parametrize("mtu,eth", [(68, True), (576, False), (1500, False)])
def test_helper_returns_the_datagrams_the_builders_cut(mtu, eth):
    """Shuffled groups of F.tx_pair: every datagram's IP payload comes back, len == T, and the span is the
    L4 payload pktgen put in."""
    rng = np.random.default_rng(mtu)
    small = mtu == 68
    dgs = F.datagrams(rng, 16, 60 if small else 600, 900 if small else 8000)
    _, ref, groups = F.tx_pair(dgs, mtu, eth, shuffle_rng=rng)
    kind = E.KIND_ETH if eth else E.KIND_IP
    offs, pos = [], 5
    for d in dgs:
        offs.append(pos)
        pos += len(d) - 20
    dg, arena = R.expected(ref, [kind] * len(ref), [0] * len(ref), [(f, c, 0) for f, c in groups], offs,
                           [len(d) - 20 for d in dgs], pos + 7)
    for i, d in enumerate(dgs):
        want = F.emit_whole(d, F.DEFAULT)[20:]
        assert int(dg[i]["len"]) == len(want) and dg[i]["copied"] == 1 and dg[i]["protocol"] == d[9]
        assert arena[offs[i]:offs[i] + len(want)].tobytes() == want
        if d[9] == 17:
            assert (int(dg[i]["l4_off"]), int(dg[i]["l4_len"])) == (8, len(want) - 8)
        elif d[9] == 6:
            assert (int(dg[i]["l4_off"]), int(dg[i]["l4_len"])) == (20, len(want) - 20)
        else:
            assert (int(dg[i]["l4_off"]), int(dg[i]["l4_len"])) == (0, 0)
    assert (arena[:5] == R.SENTINEL).all() and (arena[pos:] == R.SENTINEL).all()


def test_helper_zero_entry_for_broken_and_invalid_groups():
    rng = np.random.default_rng(9)
    _, ref, _ = F.tx_pair(F.datagrams(rng, 1, 2500, 2600), 576)
    n = len(ref)
    zero = np.zeros(1, R.DGRAM_DTYPE)[0]
    good, arena = _expected_one_group(ref, E.KIND_IP)
    assert good["len"] > 2500 and good["copied"] == 1 and (arena != R.SENTINEL).sum() > 2400
    cases = {
        "missing middle": [ref[i] for i in range(n) if i != 1],
        "missing last": ref[:-1],
        "duplicate": ref + [ref[1]],
        "other ident": ref[:1] + [ref[1][:4] + b"\x12\x34" + ref[1][6:]] + ref[2:],
        "two last": ref[:-1] + [ref[-1], ref[-1][:6] + bytes([ref[-1][6] & 0x1f]) + ref[-1][7:]],
        "cut short": ref[:2] + [ref[2][:-1]] + ref[3:],
    }
    for name, recs in cases.items():
        dg, arena = _expected_one_group(recs, E.KIND_IP)
        assert dg == zero and (arena == R.SENTINEL).all(), name
    assert _expected_one_group(ref, E.KIND_ETH)[0] == zero  # not Ethernet frames
    # the cap decides the copy, not the entry
    dg, arena = _expected_one_group(ref, E.KIND_IP, cap=int(good["len"]) - 1)
    assert dg["len"] == good["len"] and dg["copied"] == 0 and (arena == R.SENTINEL).all()
    # a raw socket's datagram and a UDP datagram with destination port 0 are delivered, without a span
    dg, _ = _expected_one_group(ref, E.KIND_IP, flags=E.REC_IPHDR_ONLY)
    assert dg["copied"] == 1 and dg["l4_off"] == 0 and dg["l4_len"] == 0
    u = P.ipv4(F.A, F.B, 17, P.udp(7, 0, bytes(100)))
    dg, _ = _expected_one_group([u], E.KIND_IP)
    assert (int(dg["len"]), int(dg["copied"]), int(dg["l4_off"]), int(dg["l4_len"])) == (108, 1, 0, 0)
    # invalid groups: outside the batch, count 0, reserved set
    for grp in ((n, 1, 0), (n - 1, 2, 0), (0, 0, 0), (0, n, 1), (0, R.MAX_FRAGMENTS + 1, 0)):
        dg, arena = R.expected(ref, [E.KIND_IP] * n, [0] * n, [grp], [0], [1 << 20], 4000)
        assert dg[0] == zero and (arena == R.SENTINEL).all(), grp
