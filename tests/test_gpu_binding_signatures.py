"""The loaded library carries the header's signatures, and the float getters that used to need a restype of their own
return what the block was constructed with.  Each getter call below is the first use of its symbol on a fresh block;
nothing but lib() has touched the function objects."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_every_declared_entry_resolves_and_carries_the_table(gpu):
    L = gpu.lib()
    table = gpu.binding.signatures()
    missing = [n for n in table if not hasattr(L, n)]
    assert not missing, "declared in grhip.h, not defined in libgrhip.so: %s" % missing
    wrong = [n for n, (restype, argtypes) in table.items()
             if getattr(L, n).restype is not restype or list(getattr(L, n).argtypes) != argtypes]
    assert not wrong, wrong


def test_fractional_interpolator_interp_ratio(gpu):
    assert gpu.fractional_interpolator_ff(0.25, 1.37).interp_ratio() == float(np.float32(1.37))


def test_logpwrfft_sample_rate(gpu):
    assert gpu.logpwrfft_c(48123.5, 64, 2.0, 30.0, 0.2, True).sample_rate() == 48123.5


def test_pwr_squelch_threshold(gpu):
    # the block keeps 10^(db / 10) and returns 10 log10 of it, in double: a few ulp of 23.5 at most (4e-15 each), so
    # 1e-12 is generous and still 13 decimal orders under what an int-typed read of the register would give
    assert abs(gpu.pwr_squelch_cc(-23.5).threshold() + 23.5) < 1e-12


def test_ctcss_squelch_level(gpu):
    assert gpu.ctcss_squelch_ff(500, 100.0, 0.0375, 250).level() == float(np.float32(0.0375))


def test_agc2_decay_rate(gpu):
    assert gpu.agc2_ff(3e-2, 2e-3).decay_rate() == float(np.float32(2e-3))
