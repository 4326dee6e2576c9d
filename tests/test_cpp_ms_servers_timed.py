"""MediaStream servers sending by the clock on the device from C++, no Python in the process
(tests/cpp/device_ms_servers_timed.cpp, built by `make`): cts_ms_server_init and cts_ms_server_schedule_init, then the
host loop of one timer over cts_media_stream_servers_send_at, every tick held against an in-program restatement of the
reference's release rule and against cts_ms_server_frames_due."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_cpp_device_ms_servers_timed():
    exe = os.path.join(ROOT, "ctstraffic_amd", "build", "device_ms_servers_timed")
    assert os.path.exists(exe), "run `make` (or __graft_entry__.build()) first"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "device_ms_servers_timed: ok" in out.stdout
