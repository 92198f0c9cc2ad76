"""ASan + UBSan over the whole-segment rule of the two-launch emit route: tests/cpp/seg_rule_asan.cpp (a
stand-alone program) includes smoltcp_amd/csrc/csum_segrule.h, the host / device function the segment pass
calls, and walks it on the CPU over every start address modulo 64, lengths 64 .. 200 and 1500, packed and
gapped strides, field offsets over the whole record, first and last records.  Host code only; any report
aborts the binary (-fno-sanitize-recover=all)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")


def test_seg_rule_walk_asan(tmp_path):
    out = str(tmp_path / "seg_rule_asan")
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, *SAN, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", out,
                    os.path.join(ROOT, "tests", "cpp", "seg_rule_asan.cpp")], check=True, timeout=300)
    r = subprocess.run([out], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.startswith("ok "), r.stdout
