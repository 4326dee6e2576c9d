"""One PushPull exchange on the device from C++, no Python in the process (tests/cpp/device_tcp_exchange.cpp, built by
`make`): cts_tcp_exchange_init, then per tick cts_tcp_exchange_send, cts_verify_at and cts_refview_accumulate_conns
over the descriptors the tick wrote, cts_conns_close of both receivers against cts_tcp_exchange_direction_bytes, and
the first ticks' descriptors, the entry and the turn against the pattern walked one buffer at a time on the host."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_cpp_device_tcp_exchange():
    exe = os.path.join(ROOT, "ctstraffic_amd", "build", "device_tcp_exchange")
    assert os.path.exists(exe), "run `make` (or __graft_entry__.build()) first"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "device_tcp_exchange: ok" in out.stdout
