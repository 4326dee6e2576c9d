"""A whole TCP exchange on the device from C++, no Python in the process (tests/cpp/device_tcp_senders.cpp, built by
`make`): cts_tcp_sender_init, then per tick cts_tcp_senders_send, cts_verify_at and cts_refview_accumulate_conns over
the descriptors the senders wrote, cts_conns_close against the transfer sizes, and two ticks' arenas and descriptors
against cts_fill over host-built descriptors."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_cpp_device_tcp_senders():
    exe = os.path.join(ROOT, "ctstraffic_amd", "build", "device_tcp_senders")
    assert os.path.exists(exe), "run `make` (or __graft_entry__.build()) first"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "device_tcp_senders: ok" in out.stdout
