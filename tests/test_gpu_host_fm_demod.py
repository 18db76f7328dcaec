"""The host-side C++ mirror of iir_filter_ffd, fm_deemph, fm_demod_cf and nbfm_rx (host/grhip_blocks.h) under the
stand-in executor: host/fm_demod_test.cc, a stand-alone program, built on demand and run once."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gnuradio-3.5.0-dmr_amd", "host")


def test_host_mirror_of_the_fm_demodulator(gpu):
    subprocess.check_call(["make", "-C", HOST, "fm_demod_test"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(HOST, "fm_demod_test")], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "fm_demod_test ok" in r.stdout, r.stdout + r.stderr
