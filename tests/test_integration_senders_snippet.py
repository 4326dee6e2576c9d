"""INTEGRATION.md's "TCP senders on the device-resident path" block compiles against include/, by the rule of
tests/test_integration_snippets.py for statement fragments: g++ -fsyntax-only, the block as a function body whose
parameters declare its free variables."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIRST = "// once per connection slot c: the sender's share of ctsIoPattern's constructor (-Transfer, -Buffer)"
PARAMS = ("cts_engine* e, void* arena, uint64_t arena_bytes, uint32_t stride, uint32_t arena_slots, "
          "const uint32_t* sending, uint32_t n_sending, uint32_t max_buffers, const uint64_t* transfer_bytes, "
          "uint32_t buffer_size, cts_tcp_sender_state* host_senders, uint32_t c, cts_tcp_sender_state* dev_senders, "
          "uint32_t n_conns, cts_buf_desc* descs, uint32_t* codes, cts_tcp_sender_tick* tick, void* sent, "
          "void* scratch, hipStream_t stream, uint32_t n_sent, uint32_t ordinal, cts_verify_result* results, "
          "void* ctr, uint32_t* conn_first_fail, void* ref, cts_conn_state* conn_state, const uint32_t* closing, "
          "const uint64_t* expected_bytes, uint32_t n_closing, cts_conn_result* close_results, void* close_ctr")
PRELUDE = r"""
#include <hip/hip_runtime_api.h>
#include "cts_tcp_senders.h"
"""


def test_senders_block_compiles():
    text = open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8").read()
    found = [code for lang, code in re.findall(r"```(\w*)\n(.*?)```", text, re.S)
             if lang == "cpp" and code.startswith(FIRST)]
    assert len(found) == 1, "INTEGRATION.md lost the senders block"
    for call in ("cts_tcp_sender_init", "cts_tcp_senders_send", "cts_verify_at", "cts_refview_accumulate_conns",
                 "cts_conns_close"):
        assert call + "(" in found[0], call
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "senders.cpp")
        with open(src, "w", encoding="utf-8") as f:
            f.write(PRELUDE + "\nvoid snippet(" + PARAMS + ")\n{\n" + found[0] + "\n}\n")
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include",
                            "-I", os.path.join(ROOT, "include"), src], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
