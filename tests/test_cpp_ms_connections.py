"""MediaStream connections on the device-resident path from C++, no Python in the process
(tests/cpp/device_ms_connections.cpp, built by `make`): cts_ms_conn_init, cts_media_stream_fill, a flipped byte, two
batches through cts_media_stream_verify_status_at and cts_media_stream_conns_accumulate, a render tick,
cts_media_stream_conns_close and a second stream through every recycled slot, all checked in C++ against one host
cts_media_stream_client per connection."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_cpp_device_ms_connections():
    exe = os.path.join(ROOT, "ctstraffic_amd", "build", "device_ms_connections")
    assert os.path.exists(exe), "run `make` (or __graft_entry__.build()) first"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "device_ms_connections: ok" in out.stdout
