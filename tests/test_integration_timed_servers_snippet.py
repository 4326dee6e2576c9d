"""INTEGRATION.md's "The frame schedule on the device-resident path" block compiles against include/, by the rule of
tests/test_integration_snippets.py for statement fragments: g++ -fsyntax-only, the block as a function body whose
parameters declare its free variables."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIRST = "// once per connection slot c: the schedule's share of ctsIoPatternMediaStreamServer"
PARAMS = ("cts_engine* e, void* ring, uint64_t ring_bytes, uint32_t stride, uint32_t ring_slots, const uint32_t* all_ids, "
          "const cts_media_stream_settings* settings, cts_ms_server_state* host_servers, "
          "cts_ms_server_schedule* host_schedule, int64_t base_time_ms, uint32_t c, cts_ms_server_state* dev_servers, "
          "cts_ms_server_schedule* dev_schedule, uint32_t n_conns, uint32_t max_frames, int64_t now_ms, int64_t qpf, "
          "cts_buf_desc* descs, uint32_t* lengths, uint32_t* codes, cts_ms_server_timed_tick* dev_tick, void* udp, "
          "void* scratch, hipStream_t stream, uint32_t ordinal, cts_datagram_status* status, void* ctr, "
          "uint32_t* conn_first_fail, cts_ms_conn_state* conns, uint64_t* frame_bytes, uint64_t frame_elems, "
          "void* udp_clients")
PRELUDE = r"""
#include <hip/hip_runtime_api.h>
#include "cts_media_stream_servers.h"
typedef struct { int64_t QuadPart; } LARGE_INTEGER;
int QueryPerformanceCounter(LARGE_INTEGER*);
int64_t sleep_until(int64_t ms);  // the caller's timer: returns the time it woke at
"""


def test_timed_servers_block_compiles():
    text = open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8").read()
    assert "## The frame schedule on the device-resident path" in text
    found = [code for lang, code in re.findall(r"```(\w*)\n(.*?)```", text, re.S)
             if lang == "cpp" and code.startswith(FIRST)]
    assert len(found) == 1, "INTEGRATION.md lost the frame schedule block"
    for call in ("cts_ms_server_schedule_init", "cts_media_stream_servers_send_at",
                 "cts_media_stream_servers_timed_scratch_bytes", "cts_ms_server_timed_tick", "next_due_ms",
                 "cts_media_stream_verify_status_at", "cts_media_stream_conns_accumulate", "sleep_until"):
        assert call in found[0], call
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "timed_servers.cpp")
        with open(src, "w", encoding="utf-8") as f:
            f.write(PRELUDE + "\nvoid snippet(" + PARAMS + ")\n{\n" + found[0] + "\n}\n")
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include",
                            "-I", os.path.join(ROOT, "include"), src], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
