"""The frame schedule's closed form under UndefinedBehaviorSanitizer and AddressSanitizer: the header that the host
helper and the planning kernels share (ctstraffic_amd/csrc/cts_ms_server_schedule_math.hpp), included by a stand-alone
program with its own main (tests/cpp/ms_server_schedule_edges.cpp) that runs the edge grid of
tests/test_media_stream_servers_timed_cpu.py: rates from 1 to 2^32 - 1, a base at the top of [0, 2^62), the last frames
of a stream of 2^32 - 1, both sides of the "< 2" rule and of final x 1000 / fps. It must exit 0 with no report."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0:exitcode=23",
       "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1:exitcode=24"}


def test_schedule_math_under_ubsan_and_asan():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "ms_server_schedule_edges")
        subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=undefined,address",
                        "-fno-sanitize-recover", "-I", os.path.join(ROOT, "ctstraffic_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "ms_server_schedule_edges.cpp"), "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, timeout=300, env={**os.environ, **ENV})
        assert out.returncode == 0, (out.returncode, out.stdout[-1000:], out.stderr[-4000:])
        assert "ms_server_schedule_edges: ok" in out.stdout
        assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
