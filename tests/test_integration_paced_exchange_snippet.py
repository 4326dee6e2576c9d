"""INTEGRATION.md's "Send pacing for every pattern on the device-resident path" block compiles against include/, by
the rule of tests/test_integration_snippets.py for statement fragments: g++ -fsyntax-only, the block as a function
body whose parameters declare its free variables."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIRST = "// once per connection slot c: both sides' pacing share of ctsIoPattern's constructor"
PARAMS = ("cts_engine* e, void* arena, uint64_t arena_bytes, uint32_t stride, uint32_t arena_slots, "
          "const uint32_t* all_ids, uint32_t max_buffers, uint64_t client_bytes_per_second, "
          "uint32_t client_burst_count, uint32_t client_burst_delay_ms, uint64_t server_bytes_per_second, "
          "uint32_t server_burst_count, uint32_t server_burst_delay_ms, cts_tcp_sender_pace* host_pace, uint32_t c, "
          "cts_tcp_exchange_state* dev_entries, cts_tcp_sender_pace* dev_pace, uint32_t n_conns, int64_t now_ms, "
          "cts_buf_desc* descs, uint32_t* codes, cts_tcp_exchange_paced_tick* dev_paced_tick, void* sent, "
          "void* scratch, hipStream_t stream, uint32_t ordinal, cts_verify_result* results, void* ctr, "
          "uint32_t* conn_first_fail, void* ref, cts_conn_state* conn_state")
PRELUDE = r"""
#include <hip/hip_runtime_api.h>
#include "cts_tcp_exchange.h"
"""


def test_paced_exchange_block_compiles():
    text = open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8").read()
    assert "## Send pacing for every pattern on the device-resident path" in text
    found = [code for lang, code in re.findall(r"```(\w*)\n(.*?)```", text, re.S)
             if lang == "cpp" and code.startswith(FIRST)]
    assert len(found) == 1, "INTEGRATION.md lost the paced exchange block"
    for call in ("cts_tcp_sender_pace_init", "host_pace[c + n_conns]", "cts_tcp_exchange_send_paced",
                 "cts_tcp_exchange_paced_scratch_bytes", "cts_tcp_exchange_paced_tick", "next_due_ms", "cts_verify_at",
                 "cts_refview_accumulate_conns", "2 * n_conns"):
        assert call in found[0], call
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "paced_exchange.cpp")
        with open(src, "w", encoding="utf-8") as f:
            f.write(PRELUDE + "\nvoid snippet(" + PARAMS + ")\n{\n" + found[0] + "\n}\n")
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include",
                            "-I", os.path.join(ROOT, "include"), src], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
