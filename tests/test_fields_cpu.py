"""CPU-side checks of emit_fields' host half: the two new ABI symbols, the 16-byte entry in its three
spellings (C, ctypes, numpy), the argument errors of smol_csum_batch_emit_fields and
smol_csum_apply_fields / engine.apply_fields.  No kernel is launched here."""
import ctypes
import os
import re

import numpy as np

import smoltcp_amd
from smoltcp_amd import _lib
from smoltcp_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _entry(off, val, status=0):
    f = _lib.FieldsC()
    for i in range(3):
        f.off[i], f.val[i] = off[i], val[i]
    f.status = status
    return f


def _apply(rec: np.ndarray, length: int, f) -> int:
    return smoltcp_amd.lib().smol_csum_apply_fields(rec.ctypes.data, length, ctypes.byref(f))


def test_symbols_declared_and_exported():
    with open(os.path.join(ROOT, "include", "smolcsum.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    L = smoltcp_amd.lib()
    for name in ("smol_csum_batch_emit_fields", "smol_csum_apply_fields"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(L, name) and name in _lib.ABI_SYMBOLS
    assert "smol_csum_fields_t" in text and re.search(r"#define\s+SMOL_NO_FIELD\s+0xffffu", text)
    with open(os.path.join(ROOT, "include", "smolcsum_tools.h")) as f:
        assert "smol_csum_tool_set_fields_kernel" in f.read()
    assert hasattr(L, "smol_csum_tool_set_fields_kernel") and "smol_csum_tool_set_fields_kernel" in _lib.TOOL_SYMBOLS
    assert L.smol_csum_abi_version() == 6  # additive: the version stays


def test_entry_is_16_bytes_in_every_spelling():
    assert ctypes.sizeof(_lib.FieldsC) == 16
    assert E.FIELDS_DTYPE.itemsize == 16
    f = _entry((1, 2, 3), (0x0405, 0x0607, 0x0809), 0x60)
    a = np.frombuffer(bytes(f), dtype=E.FIELDS_DTYPE)[0]
    assert list(a["off"]) == [1, 2, 3] and list(a["val"]) == [0x0405, 0x0607, 0x0809]
    assert a["status"] == 0x60 and not a["reserved"].any()
    assert bytes(f)[12] == 0x60 and bytes(f)[:2] == b"\x01\x00" and bytes(f)[6:8] == b"\x05\x04"


def test_emit_fields_argument_errors():
    L = smoltcp_amd.lib()
    b = _lib.BatchC()
    b.n, b.stride, b.len, b.kind = 1, 64, 64, 1
    caps = _lib.Caps()
    buf = (ctypes.c_uint8 * 64)()
    ent = (ctypes.c_uint8 * 48)()
    aligned = (ctypes.addressof(ent) + 15) & ~15
    ctx = ctypes.c_void_p(1)  # never dereferenced: every case below fails its argument checks first
    call = L.smol_csum_batch_emit_fields
    assert call(None, buf, ctypes.byref(b), ctypes.byref(caps), aligned, None) == _lib.SMOL_EINVAL  # NULL ctx
    assert call(ctx, buf, ctypes.byref(b), ctypes.byref(caps), None, None) == _lib.SMOL_EINVAL  # NULL d_fields
    assert call(ctx, buf, ctypes.byref(b), ctypes.byref(caps), aligned + 8, None) == _lib.SMOL_EINVAL  # misaligned
    assert call(ctx, buf, ctypes.byref(b), None, aligned, None) == _lib.SMOL_EINVAL  # NULL caps
    bad = _lib.Caps()
    bad.udp = 4
    assert call(ctx, buf, ctypes.byref(b), ctypes.byref(bad), aligned, None) == _lib.SMOL_EINVAL  # bad caps value
    bad = _lib.Caps()
    bad.reserved[1] = 1
    assert call(ctx, buf, ctypes.byref(b), ctypes.byref(bad), aligned, None) == _lib.SMOL_EINVAL
    b.n = 0  # nothing to do: OK whatever d_fields is, SMOL_BATCH_FIELD_STORES accepted
    b.flags = 0x80
    assert call(ctx, None, ctypes.byref(b), ctypes.byref(caps), None, None) == _lib.SMOL_OK
    assert L.smol_csum_tool_set_fields_kernel(None, 0) == _lib.SMOL_EINVAL


def test_apply_fields_writes_big_endian_and_skips_no_field():
    rec = np.arange(64, dtype=np.uint8)
    want = rec.copy()
    f = _entry((10, 26, _lib.NO_FIELD), (0x1234, 0xABCD, 0x5555))
    assert _apply(rec, 64, f) == _lib.SMOL_OK
    want[10:12] = (0x12, 0x34)
    want[26:28] = (0xAB, 0xCD)
    assert np.array_equal(rec, want)
    # odd offsets, all three fields, the last one ending at the record's last byte
    f = _entry((1, 33, 62), (0x0102, 0xFFFF, 0x00FE))
    assert _apply(rec, 64, f) == _lib.SMOL_OK
    want[1:3] = (1, 2)
    want[33:35] = (0xFF, 0xFF)
    want[62:64] = (0, 0xFE)
    assert np.array_equal(rec, want)
    # no field at all: nothing written
    assert _apply(rec, 0, _entry((_lib.NO_FIELD,) * 3, (7, 7, 7))) == _lib.SMOL_OK
    assert np.array_equal(rec, want)


def test_apply_fields_erange_leaves_the_record_unchanged():
    for bad_slot in range(3):
        for off, length in ((63, 64), (64, 64), (0, 1), (0, 0), (0xFFFE, 64), (10, 11)):
            rec = np.full(80, 0x5A, dtype=np.uint8)
            offs, vals = [4, 20, 40], [0x1111, 0x2222, 0x3333]
            offs[bad_slot] = off
            good_len = max(length, 0)
            # the other two fields fit only when the record is long enough: keep them inside `length`
            for j in range(3):
                if j != bad_slot and offs[j] + 2 > length:
                    offs[j] = _lib.NO_FIELD
            assert _apply(rec, good_len, _entry(offs, vals)) == _lib.SMOL_ERANGE, (bad_slot, off, length)
            assert (rec == 0x5A).all(), (bad_slot, off, length)
    L = smoltcp_amd.lib()
    assert L.smol_csum_apply_fields(None, 4, ctypes.byref(_entry((0, 0, 0), (0, 0, 0)))) == _lib.SMOL_EINVAL


def test_numpy_apply_fields_agrees_with_c():
    rng = np.random.default_rng(0xF1E1D5)
    n = 1000
    lens = rng.integers(0, 200, n).astype(np.int64)
    offs = np.concatenate(([0], np.cumsum(lens[:-1] + rng.integers(0, 5, n - 1)))).astype(np.int64)
    total = int(offs[-1] + lens[-1]) + 8
    f = np.zeros(n, dtype=E.FIELDS_DTYPE)
    # three distinct, non-overlapping slots per record at even or odd offsets; a share absent, a share
    # out of range (past the record, or straddling its end)
    base = rng.integers(0, 60, n)
    for j in range(3):
        o = base + 64 * j + rng.integers(0, 30, n) * 2 + rng.integers(0, 2, n)
        o = np.where(rng.random(n) < 0.3, _lib.NO_FIELD, o)
        f["off"][:, j] = o
        f["val"][:, j] = rng.integers(0, 65536, n)
    edge = rng.random(n) < 0.1  # a field that ends exactly at, or one byte past, the record's end
    pick = np.flatnonzero(edge & (lens >= 2))
    f["off"][pick, 1] = lens[pick] - 2 + rng.integers(0, 2, len(pick))
    f["off"][pick, 0] = f["off"][pick, 2] = _lib.NO_FIELD  # (fields never overlap)
    f["status"] = rng.integers(0, 256, n)
    host_c = rng.integers(0, 256, total, dtype=np.uint8)
    host_np = host_c.copy()
    L = smoltcp_amd.lib()
    rc = np.empty(n, dtype=np.int64)
    ent = f.view(np.uint8).reshape(n, 16)
    for i in range(n):
        rec = host_c[offs[i]:]
        rc[i] = L.smol_csum_apply_fields(rec.ctypes.data, int(lens[i]), ent[i].ctypes.data_as(ctypes.POINTER(_lib.FieldsC)))
    ok = E.apply_fields(host_np, offs, lens, f)
    assert set(np.unique(rc)) <= {_lib.SMOL_OK, _lib.SMOL_ERANGE}
    assert (rc == _lib.SMOL_ERANGE).sum() > 50 and (rc == _lib.SMOL_OK).sum() > 50
    assert np.array_equal(ok, rc == _lib.SMOL_OK)
    assert np.array_equal(host_np, host_c)
    # the n x 16 uint8 spelling, and a scalar record length
    host2 = np.zeros(64 * 8, dtype=np.uint8)
    g = np.zeros(8, dtype=E.FIELDS_DTYPE)
    g["off"] = _lib.NO_FIELD
    g["off"][:, 1] = 26
    g["val"][:, 1] = np.arange(8) + 0x0100
    assert E.apply_fields(host2, np.arange(8) * 64, 64, g.view(np.uint8).reshape(8, 16)).all()
    assert list(host2.reshape(8, 64)[:, 26]) == [1] * 8 and list(host2.reshape(8, 64)[:, 27]) == list(range(8))
