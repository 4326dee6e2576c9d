"""A whole MediaStream exchange on the device from C++, no Python in the process (tests/cpp/device_ms_servers.cpp,
built by `make`): cts_ms_server_init and cts_ms_conn_init, then per tick cts_media_stream_servers_send,
cts_media_stream_verify_status_at, cts_media_stream_conns_accumulate and cts_media_stream_conns_render over the
descriptors the servers wrote, the close, and one tick's ring against cts_media_stream_fill_strided's."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_cpp_device_ms_servers():
    exe = os.path.join(ROOT, "ctstraffic_amd", "build", "device_ms_servers")
    assert os.path.exists(exe), "run `make` (or __graft_entry__.build()) first"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "device_ms_servers: ok" in out.stdout
