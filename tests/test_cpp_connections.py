"""The connection lifecycle on the device-resident path from C++, no Python in the process
(tests/cpp/device_connections.cpp, built by `make`): cts_fill, corruptions, cts_verify_at,
cts_refview_accumulate_conns, cts_conn_slots_rebase, cts_conns_close and a second connection through every recycled
slot, all checked in C++ against values computed there."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_cpp_device_connections():
    exe = os.path.join(ROOT, "ctstraffic_amd", "build", "device_connections")
    assert os.path.exists(exe), "run `make` (or __graft_entry__.build()) first"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "device_connections: ok" in out.stdout
