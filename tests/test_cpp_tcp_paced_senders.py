"""A paced TCP exchange on the device from C++, no Python in the process (tests/cpp/device_tcp_paced_senders.cpp,
built by `make`): cts_tcp_sender_pace_init, then per tick cts_tcp_senders_send_paced, cts_verify_at and
cts_refview_accumulate_conns over the descriptors the senders wrote, the clock moved to the tick block's next_due_ms,
and cts_conns_close against the transfer sizes; the times of every connection's last send are the settings'."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_cpp_device_tcp_paced_senders():
    exe = os.path.join(ROOT, "ctstraffic_amd", "build", "device_tcp_paced_senders")
    assert os.path.exists(exe), "run `make` (or __graft_entry__.build()) first"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "device_tcp_paced_senders: ok" in out.stdout
