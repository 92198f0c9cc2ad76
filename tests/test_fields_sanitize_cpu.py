"""ASan + UBSan over emit_fields' host half: tests/cpp/fields_asan.cpp (a stand-alone program) compiled
together with smoltcp_amd/csrc/csum_scalar.cpp under -fsanitize=address,undefined, driving
smol_csum_apply_fields over records that sit in heap blocks of exactly their length, the SMOL_ERANGE paths
included.  Host code only; any report aborts the binary (-fno-sanitize-recover=all)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fields_asan") / "fields_asan")
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, *SAN, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", out,
                    os.path.join(ROOT, "tests", "cpp", "fields_asan.cpp"),
                    os.path.join(ROOT, "smoltcp_amd", "csrc", "csum_scalar.cpp")], check=True, timeout=300)
    return out


@pytest.mark.parametrize("seed", [1, 0xF1E1D5])
def test_apply_fields_asan(binary, seed):
    r = subprocess.run([binary, str(seed), "20000"], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip() == "ok 20000"
