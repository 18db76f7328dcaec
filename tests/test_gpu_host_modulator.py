"""The host-side C++ mirror of packed_to_unpacked_bb, unpacked_to_packed_bb, diff_encoder_bb, chunks_to_symbols_bc and
generic_mod (host/grhip_blocks.h) under the stand-in executor: host/modulator_test.cc, a stand-alone program, built on
demand and run once."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gnuradio-3.5.0-dmr_amd", "host")


def test_host_mirror_of_the_modulator_blocks(gpu):
    subprocess.check_call(["make", "-C", HOST, "modulator_test"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(HOST, "modulator_test")], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "modulator_test ok" in r.stdout, r.stdout + r.stderr
