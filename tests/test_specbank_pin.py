"""oracle.cubicsdr_chain.RefSpectrum -- the checker of the spectrum bank's tests -- fed inputs of VARYING length, against the reference's own
src/process/SpectrumVisualProcessor.cpp (oracle/_ref/libref_spectrum.so), bit for bit: which inputs produce output, the points, the held points,
fft_ceiling / fft_floor.  The existing pin (tests/test_oracle_pin.py) feeds fixed lengths only; the bank's cases (tests/specbank_cases.py) cross every
branch of the frame selection (:387-421) from input to input, with peak hold enabled in front of input 2 and again in front of input 5."""
import numpy as np
import pytest

from tests import specbank_cases as K


def _same(a, w):
    """the same floats bit for bit; a NaN equals a NaN (its sign bit is whatever the last operation left: no statement of the reference reads it)"""
    a, w = np.asarray(a), np.asarray(w)
    nan = np.isnan(w)
    return a.shape == w.shape and np.array_equal(np.isnan(a), nan) and a[~nan].tobytes() == w[~nan].tobytes()


@pytest.mark.parametrize("peak", [False, True])
@pytest.mark.parametrize("F", K.SIZES)
def test_ref_spectrum_with_varying_input_lengths_equals_the_reference_class(F, peak):
    from oracle import ref_modems as RM
    from oracle.cubicsdr_chain import RefSpectrum
    if not RM.spectrum_available():
        pytest.skip("oracle/_ref/libref_spectrum.so is built only where the reference tree is present")
    n_items = sum(K.PEAK_CALLS) if peak else K.N_ITEMS
    data = K.make_inputs(F, n_items, nan=not peak)
    freq, rate = 100000000, 2400000
    nout = nhold = 0
    for s in sorted(data):
        if data[s] is None:
            continue
        cpp = RM.RefSpectrumCpp(F, rate)
        cpp.set_center(freq); cpp.set_bandwidth(rate)
        py = RefSpectrum("ref", F)
        try:
            for k, x in enumerate(data[s]):
                if peak and k in (2, 5):
                    cpp.set_peak_hold(True); py.set_peak_hold(True)
                if len(x) == 0:
                    continue                            # the library's own definition: no input at all (neither class sees it)
                a, w = cpp.process(x, freq, rate), py.process_input(x)
                assert (a is None) == (w is None), (F, s, k)
                if a is None:
                    continue
                nout += 1
                assert _same(a[0], w[0]), (F, s, k)
                assert _same(np.float64([a[1], a[2]]), np.float64([w[1], w[2]])), (F, s, k)
                assert (a[3] is None) == (w[3] is None), (F, s, k)
                if a[3] is not None:
                    nhold += 1
                    assert _same(a[3], w[3]), (F, s, k)
        finally:
            cpp.close()
    assert nout >= 5 * (n_items - 2) and (nhold > 20) == peak
