"""One rate-limited PushPull exchange on the device from C++, no Python in the process
(tests/cpp/device_tcp_paced_exchange.cpp, built by `make`): cts_tcp_exchange_init, a pace entry per side from
cts_tcp_sender_pace_init, then per tick cts_tcp_exchange_send_paced at the tick block's next_due_ms, cts_verify_at and
cts_refview_accumulate_conns over the descriptors the tick wrote, cts_conns_close of both receivers, and every tick's
count, descriptors, due time and the final pace entries against the pattern walked one buffer at a time on the host
with CreateNewTask's send branch per side."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_cpp_device_tcp_paced_exchange():
    exe = os.path.join(ROOT, "ctstraffic_amd", "build", "device_tcp_paced_exchange")
    assert os.path.exists(exe), "run `make` (or __graft_entry__.build()) first"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "device_tcp_paced_exchange: ok" in out.stdout
