"""The host-side C++ mirror of the trellis blocks (host/grhip_blocks.h): host/trellis_test.cc, a stand-alone program,
built on demand and run once."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gnuradio-3.5.0-dmr_amd", "host")


def test_host_mirror_of_the_trellis_blocks(gpu):
    subprocess.check_call(["make", "-C", HOST, "trellis_test"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(HOST, "trellis_test")], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "trellis_test ok" in r.stdout, r.stdout + r.stderr
