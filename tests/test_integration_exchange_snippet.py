"""INTEGRATION.md's "Pull, PushPull and Duplex on the device-resident path" block compiles against include/, by the
rule of tests/test_integration_snippets.py for statement fragments: g++ -fsyntax-only, the block as a function body
whose parameters declare its free variables."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIRST = "// once per connection slot c: the pattern's share of ctsIoPattern's constructor"
PARAMS = ("cts_engine* e, void* arena, uint64_t arena_bytes, uint32_t stride, uint32_t arena_slots, "
          "const uint32_t* listed, uint32_t n_listed, uint32_t max_buffers, uint64_t transfer_bytes, "
          "uint32_t buffer_size, uint32_t push_bytes, uint32_t pull_bytes, cts_tcp_exchange_state* host_entries, "
          "uint32_t c, uint64_t* expected_bytes, cts_tcp_exchange_state* dev_entries, uint32_t n_conns, "
          "cts_buf_desc* descs, uint32_t* codes, cts_tcp_exchange_tick* dev_tick, void* sent, void* scratch, "
          "hipStream_t stream, uint32_t n_sent, uint32_t ordinal, cts_verify_result* results, void* ctr, "
          "uint32_t* conn_first_fail, void* ref, cts_conn_state* conn_state, uint64_t taken, uint32_t direction, "
          "uint32_t intra_segment_transfer, const uint32_t* closing, const uint64_t* expected_bytes_of_closing, "
          "uint32_t n_closing, cts_conn_result* close_results, void* close_ctr")
PRELUDE = r"""
#include <hip/hip_runtime_api.h>
#include "cts_tcp_exchange.h"
"""


def test_exchange_block_compiles():
    text = open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8").read()
    assert "## Pull, PushPull and Duplex on the device-resident path" in text
    found = [code for lang, code in re.findall(r"```(\w*)\n(.*?)```", text, re.S)
             if lang == "cpp" and code.startswith(FIRST)]
    assert len(found) == 1, "INTEGRATION.md lost the exchange block"
    for call in ("cts_tcp_exchange_init", "cts_tcp_exchange_direction_bytes", "cts_tcp_exchange_send",
                 "cts_tcp_exchange_scratch_bytes", "cts_tcp_exchange_seek", "cts_tcp_exchange_where", "cts_verify_at",
                 "cts_refview_accumulate_conns", "cts_conns_close", "2 * n_conns"):
        assert call in found[0], call
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "exchange.cpp")
        with open(src, "w", encoding="utf-8") as f:
            f.write(PRELUDE + "\nvoid snippet(" + PARAMS + ")\n{\n" + found[0] + "\n}\n")
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include",
                            "-I", os.path.join(ROOT, "include"), src], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
