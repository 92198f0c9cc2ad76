"""CPU-side checks of the C-ABI library: it loads, exports every symbol the headers declare, the
scalar host mirrors are bit-exact against the oracle, and the batched entry points fail loudly
(no CPU fallback) without a GPU.  No kernel is launched here."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import oracle
from oracle import pyref
import smoltcp_amd
from smoltcp_amd import _lib, checksum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    with open(os.path.join(ROOT, "include", header)) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(smol_csum_\w+)\s*\(", text)))


def test_library_loads_and_exports_all_declared_symbols():
    L = smoltcp_amd.lib()
    decl = _declared("smolcsum.h") + _declared("smolcsum_tools.h")
    assert len(decl) >= 17
    for name in decl:
        assert hasattr(L, name), f"{name} declared in include/ but not exported"
    assert sorted(_lib.ABI_SYMBOLS) == _declared("smolcsum.h")
    assert sorted(_lib.TOOL_SYMBOLS) == _declared("smolcsum_tools.h")
    assert L.smol_csum_abi_version() == 6


def test_library_is_a_gfx950_code_object():
    with open(_lib.LIB_PATH, "rb") as f:
        blob = f.read()
    assert b"gfx950" in blob, "libsmolcsum.so must embed gfx950 device code"


def test_scalar_data_matches_oracle():
    rng = np.random.default_rng(1)
    cases = [b"", b"\x01", b"\xff\xff", bytes(131074), b"\xff" * 131075, b"\xff" * 300001]
    cases += [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in range(0, 200)]
    cases += [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (1500, 9000, 65535)]
    for c in cases:
        assert checksum.data(c) == oracle.data(c), len(c)


def test_scalar_combine_and_pseudo_headers():
    rng = np.random.default_rng(2)
    for _ in range(300):
        ws = [int(x) for x in rng.integers(0, 65536, int(rng.integers(0, 8)))]
        assert checksum.combine(ws) == pyref.combine(ws)
        s4, d4 = rng.integers(0, 256, 4, dtype=np.uint8).tobytes(), rng.integers(0, 256, 4, dtype=np.uint8).tobytes()
        s6, d6 = rng.integers(0, 256, 16, dtype=np.uint8).tobytes(), rng.integers(0, 256, 16, dtype=np.uint8).tobytes()
        p, ln = int(rng.integers(256)), int(rng.integers(0, 1 << 32))
        assert checksum.pseudo_header_v4(s4, d4, p, ln) == pyref.pseudo_header_v4(s4, d4, p, ln)
        assert checksum.pseudo_header_v6(s6, d6, p, ln) == pyref.pseudo_header_v6(s6, d6, p, ln)
        assert checksum.pseudo_header(s4, d4, p, ln) == pyref.pseudo_header(s4, d4, p, ln)
        assert checksum.pseudo_header(s6, d6, p, ln) == pyref.pseudo_header(s6, d6, p, ln)
    with pytest.raises(ValueError):
        checksum.pseudo_header(bytes(4), bytes(16), 6, 0)


def test_scalar_mirrors_on_kats(golden):
    """data() of each KAT span (with its pseudo-header) reproduces the reference verdict."""
    for k in golden["kat"]:
        b = bytes.fromhex(k["bytes"])
        if k["proto"] == "ipv4":
            assert checksum.data(b[: (b[0] & 15) * 4]) == 0xFFFF
        elif k["proto"] in ("icmpv4", "igmp"):
            assert checksum.data(b) == 0xFFFF
        elif k["proto"] == "udp" and k["checksum"] == 0:
            continue
        else:
            src, dst = bytes.fromhex(k["src"]), bytes.fromhex(k["dst"])
            pnum = {"udp": 17, "tcp": 6, "icmpv6": 58}[k["proto"]]
            ln = (b[4] << 8 | b[5]) if k["proto"] == "udp" else len(b)
            span = b[:ln]
            if k["name"] == "udp4_zero_checksum":
                continue
            assert checksum.combine([checksum.pseudo_header(src, dst, pnum, ln), checksum.data(span)]) == 0xFFFF, k["name"]


def test_batched_calls_fail_loudly_without_a_device():
    L = smoltcp_amd.lib()
    h = ctypes.c_void_p()
    rc = L.smol_csum_ctx_create(0, ctypes.byref(h))
    try:
        import torch

        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if not has_gpu:
        assert rc == _lib.SMOL_ENODEV
    else:
        assert rc == _lib.SMOL_OK
        L.smol_csum_ctx_destroy(h)
    b = _lib.BatchC()
    b.n = 1
    caps = _lib.Caps()
    st = ctypes.c_uint8()
    assert L.smol_csum_batch_verify(None, None, ctypes.byref(b), ctypes.byref(caps), ctypes.byref(st), None) == _lib.SMOL_EINVAL
    assert L.smol_csum_batch_emit(None, None, ctypes.byref(b), ctypes.byref(caps), None, None) == _lib.SMOL_EINVAL
    assert L.smol_csum_batch_data(None, None, ctypes.byref(b), None, None) == _lib.SMOL_EINVAL
    with pytest.raises(Exception):
        from smoltcp_amd.engine import ChecksumEngine

        if not has_gpu:
            ChecksumEngine(0)
        else:
            raise RuntimeError("skip: GPU present")


def test_auto_shape():
    from smoltcp_amd.engine import auto_shape

    assert auto_shape(64) == 0      # 8 lanes x 6 chunks
    assert auto_shape(1500) == 7    # 8 x 7: eight 1500-byte records per wavefront, two steps each
    assert auto_shape(1900) == 4    # 32 x 4 (line grid: up to 2048 - 127 bytes)
    assert auto_shape(9000) == 6    # 64 x 4
    assert auto_shape(1500, True) == 8  # descriptors: 16 x 4 (verify: line grid, no prefetch)


def test_phy_policy_mirror():
    from smoltcp_amd.phy import Checksum, ChecksumCapabilities

    assert Checksum.Both.rx() and Checksum.Both.tx()
    assert Checksum.Rx.rx() and not Checksum.Rx.tx()
    assert Checksum.Tx.tx() and not Checksum.Tx.rx()
    assert not Checksum.None_.rx() and not Checksum.None_.tx()
    assert ChecksumCapabilities().as_tuple() == (0, 0, 0, 0, 0)
    assert ChecksumCapabilities.ignored().as_tuple() == (3, 3, 3, 3, 3)


def test_variant_lists():
    """The product library runs the defaults and one fallback per operation; the experiments build
    (when it has been built) every measured variant besides (csum_api.cpp variant_built)."""
    from smoltcp_amd import _lib

    L = _lib.lib()
    built = [v for v in range(-1, 128) if L.smol_csum_tool_variant_built(v)]
    assert built == [-1, 5, 7, 13, 17, 21, 39, 41, 44, 47, 57, 60, 63, 89, 97, 101], built
    if os.path.exists(_lib.EXP_LIB_PATH):
        X = _lib.lib(_lib.EXP_LIB_PATH)
        exp = {v for v in range(-1, 128) if X.smol_csum_tool_variant_built(v)}
        assert set(built) < exp and {0, 1, 3, 4, 16, 19, 23, 28, 29, 31, 37, 38, 42, 56, 80, 81, 82, 83, 64 + 37, 64 + 44, 64 + 47} <= exp


def test_dispatch_table_matches_sweeps():
    """smoltcp_amd/csrc/dispatch_table.inc (the fixed-stride dispatch, csum_api.cpp xwalk_auto) is what
    tools/gen_dispatch_table.py makes from the committed length sweeps (profiles/r06_dispatch_sweep_*),
    and C2's 1500-B records take the transposed walk with the first-load hint (verify) and with
    non-temporal write-through segments (emit, 101: the sweep's 57 with write-through stores)."""
    import subprocess

    from tests.dispatch_table import fixed_launch

    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_dispatch_table.py"), "--check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert fixed_launch("verify", 1500, 1500) == ("xwalk_kernel", 89)
    assert fixed_launch("emit", 1500, 1500) == ("xwalk_kernel", 101)
    assert fixed_launch("verify", 1000, 1000) == ("csum_kernel", 5)


def _both_libs():
    assert os.path.exists(_lib.EXP_LIB_PATH), "build() makes the experiments library too"
    return (("product", _lib.lib()), ("experiments", _lib.lib(_lib.EXP_LIB_PATH)))


def test_dispatch_matches_recorded_dump():
    """smol_csum_tool_pick (csum_dispatch.h pick_kernel) decides what the commit before the variant
    registry decided.  tests/data/dispatch_dump_parent.txt.gz was recorded from that commit, never from
    the code under test: its pick_kernel behind the same context-free entry, both of its libraries,
    tests/dispatch_dump.py's grid (every built variant, desc_staged, a forced shape, the four ops, packed
    / gapped by 1 / gapped by 64 / descriptor batches, SMOL_BATCH_FIELD_STORES, SMOL_REC_IPHDR_ONLY, NHC)
    at lengths 64, 1500, 1922 and 9024, then run-length coded as text (the full 25-length dump was compared once, when the registry
    went in)."""
    from tests import dispatch_dump as D

    want = list(D.recorded_lines(os.path.join(ROOT, "tests", "data", "dispatch_dump_parent.txt")))
    got = [line for name, L in _both_libs() for line in D.dump_lines(L, name, D.RECORDED_LENGTHS)]
    assert len(want) == 60416 and len(got) == len(want)
    bad = [(w, g) for w, g in zip(want, got) if w != g]
    assert not bad, (len(bad), bad[:5])


def test_kernel_forms_match_recorded_table():
    """The registry's (variant, mode) -> kernel form (smol_csum_tool_form: the switch the launchers
    instantiate xwalk_kernel / dwalk_kernel through) is the one the commit before the registry launched.
    tests/data/kernel_forms_parent.jsonl was recorded from that commit: its launch_xwalk and
    launch_dwalk compiled for the host with the launch macro recording the kernel's template arguments,
    grid and block, called for every variant, both modes and every R (100000 records of 1409, 1500,
    1922, 3970 and 8066 B), with and without SMOL_EXP, normalised to named values and restricted to the
    (variant, mode) pairs that commit's dispatch could deliver.  Its product rows no longer include the
    staged forms of 94 / 95 / 96, which the product library never ran."""
    import json

    with open(os.path.join(ROOT, "tests", "data", "kernel_forms_parent.jsonl")) as f:
        want = [json.loads(line) for line in f]
    xnames = ["NOSTORE", "SEG", "PERSIST", "NTS", "HALF", "STAGE", "HINT", "WPE", "WV", "STEPS"]
    plain = dict(zip(xnames, [0, 0, 0, 0, 0, 0, 0, 0, 4, 1]))
    out = (ctypes.c_int * 13)()
    info = (ctypes.c_int * 4)()
    for name, L in _both_libs():
        rows = [r for r in want if r["lib"] == name]
        assert rows
        seen = set()
        for r in rows:
            op = 1 if r["mode"] == "emit" else 2
            assert r["kernel_mode"] == r["mode"]
            assert L.smol_csum_tool_form(r["variant"], op, out) == 0, (name, r["variant"], r["mode"])
            seen.add((r["variant"], op))
            then = [t["kernel"] for t in r["then"]]
            if r["family"] == "xwalk":
                assert out[0] == 2
                form = dict(zip(xnames, out[1:11]))
                only_r, max_len = out[11], out[12]
                if (only_r and only_r != r["R"]) or (max_len and r["len"] > max_len):
                    form = plain
                assert form == r["form"], (name, r["variant"], r["mode"], r["len"], form, r["form"])
                assert r["block"] == 64 * form["WV"]
                if not form["PERSIST"]:
                    wgs = -(-100000 // (4 * r["R"]))
                    assert r["grid"] == -(-wgs // (form["WV"] // 4 * form["STEPS"]))
                assert then == (["seg_pass4_kernel"] if form["STAGE"] else [])
            else:
                assert out[0] == 3
                form = dict(zip(["NOSTORE", "GROUPS", "SEGF"], out[1:4]))
                assert form == r["form"], (name, r["variant"], r["mode"], form, r["form"])
                assert then == {-1: [], 0: ["seg_pass4_kernel"], 1: ["seg_pass_kernel"]}[out[4]]
        # and the library has no form the recorded commit did not launch
        for v in range(128):
            for op in (1, 2):
                if L.smol_csum_tool_form(v, op, out) == 0:
                    assert (v, op) in seen, (name, v, op)
                    assert L.smol_csum_tool_variant_info(v, info) == 0 and info[0] in (2, 3) and info[2] == 1
    P = _lib.lib()
    for v in (94, 95, 96):
        assert P.smol_csum_tool_form(v, 1, out) == _lib.SMOL_EINVAL


def test_walk_launches_match_recorded_table():
    """The walk kernel's and copy_kernel's launchers (smol_csum_tool_walk_launch: the registry switches and the
    shape mappers that launch_walk / launch_walk_nhc / launch_copy_kernel run) launch what the commit before
    the named walk forms launched.
    tests/data/walk_launch_parent.jsonl was recorded from that commit, never from the code under test: a
    program linked against each of its two libraries called smolcsum::launch_csum for every variant
    0-127, data / emit / verify / copy-emit, fixed-stride and descriptor batches, NHC on and off and all
    nine launch shapes, ignored the no-device launch error and read smol_csum_tool_last_launch
    (note_launch runs before the launch), with a sentinel launch of another kernel family between probes
    to tell the calls that launch nothing apart.  One line per (library, variant, op, batch form, nhc)
    that launched anything, with the nine packed last_launch values; a missing line is an error for all
    nine.  Every line is served: the walk's, the NHC walk's and copy_kernel's (17 / 21 / 22 / 30 / 98 / 102,
    kernel id 3)."""
    import json

    want = {}
    with open(os.path.join(ROOT, "tests", "data", "walk_launch_parent.jsonl")) as f:
        for line in f:
            r = json.loads(line)
            assert len(r["launch"]) == 9
            want[(r["lib"], r["variant"], r["op"], r["implicit"], r["nhc"])] = r["launch"]
    assert len(want) == 1235
    out = (ctypes.c_int * 4)()
    served = 0
    for name, L in _both_libs():
        assert any(k[0] == name for k in want)
        for v in range(128):
            for op in range(4):
                for implicit in (1, 0):
                    for nhc in (0, 1):
                        rec = want.get((name, v, op, implicit, nhc), ["error"] * 9)
                        for shape in range(9):
                            rc = L.smol_csum_tool_walk_launch(v, op, implicit, nhc, shape, out)
                            exp = rec[shape]
                            where = (name, v, op, implicit, nhc, shape)
                            if exp != "error":
                                assert exp >> 24 in (1, 3, 4)  # KERN_WALK, KERN_COPY, KERN_WALK_NHC
                                assert rc == 0, where
                                assert out[0] << 24 | out[1] << 16 | out[2] << 8 | out[3] == exp, (where, list(out), exp)
                                served += 1
                            else:  # and the library serves nothing the recorded commit did not
                                assert rc == _lib.SMOL_EINVAL, (where, list(out))
        assert L.smol_csum_tool_walk_launch(5, 4, 1, 0, 0, out) == _lib.SMOL_EINVAL
        assert L.smol_csum_tool_walk_launch(5, 1, 1, 0, 9, out) == _lib.SMOL_EINVAL
    assert served == 9 * 1235
