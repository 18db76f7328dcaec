"""The restatements of agc2_cc, fll_band_edge_cc, pfb_clock_sync_ccf and the constellation tail in a row, on the CPU
(demod_chain_ref.py): the signal that tests/test_gpu_demod_chain.py sends through the device decodes without an error
behind the settling prefix, at its own noise level and, as the margin, at twice and at four times that level and with a
prefix of 300 symbols in place of 1024; and no other lag decodes."""
import numpy as np
import pytest

import demod_chain_ref as D


@pytest.mark.parametrize("factor", (1, 2, 4))
def test_the_restated_chain_decodes_with_margin(g, factor):
    taps = g.fll_band_edge_taps(*D.FLL[:3])
    x, v = D.transmit(noise=factor * D.NOISE)
    bits = D.restated_chain(x, taps)
    assert len(bits) % 2 == 0 and len(bits) // 2 > D.NSYM - 100
    errors, compared = D.errors_behind_prefix(bits, v, D.LAG)
    assert errors == 0 and compared > D.NSYM - D.PREFIX - 100
    got = np.asarray(bits, np.uint8).reshape(-1, 2)[300:D.PREFIX]                   # the prefix is generous
    assert np.array_equal(got, D.bits_of(v[300 - D.LAG:D.PREFIX - D.LAG]).reshape(-1, 2))
    if factor == 1:
        for lag in (D.LAG - 1, D.LAG + 1):
            assert D.errors_behind_prefix(bits, v, lag)[0] > compared // 2          # about half the bits of random data
