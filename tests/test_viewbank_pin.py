"""oracle.cubicsdr_chain.RefSpectrum in VIEW mode -- the checker of the view bank's tests -- over the walks of tests/viewbank_cases.py that leave the
ground the existing pin covers, against the reference's own src/process/SpectrumVisualProcessor.cpp (oracle/_ref/libref_spectrum.so), bit for bit:
which inputs produce output, desiredInputSize, the points, fft_ceiling / fft_floor.  Walk (b): no mixing, two half-band stages, a priming input and
sliding ones; (c): retunes that move the averagers left, right, not at all, and a repeated centre; (d): a squeeze and a stretch behind two rebuilt
resamplers; (f): a view out of range of the input."""
import numpy as np
import pytest

from tests import viewbank_cases as K


def _same(a, w):
    """the same floats bit for bit; a NaN equals a NaN"""
    a, w = np.asarray(a), np.asarray(w)
    nan = np.isnan(w)
    return a.shape == w.shape and np.array_equal(np.isnan(a), nan) and a[~nan].tobytes() == w[~nan].tobytes()


@pytest.mark.parametrize("F", (16, 32))
def test_ref_spectrum_in_view_mode_equals_the_reference_class(F):
    from oracle import ref_modems as RM
    from oracle.cubicsdr_chain import RefSpectrum
    if not RM.spectrum_available():
        pytest.skip("oracle/_ref/libref_spectrum.so is built only where the reference tree is present")
    w, data = K.walks(F), K.make_inputs(F)
    nout = 0
    for s in (K.B, K.C_, K.D, K.F_):
        cpp = RM.RefSpectrumCpp(F, K.RATE)                  # (the application rate of :306 is the input's)
        py = RefSpectrum("ref", F)
        try:
            for k, x in enumerate(data[s]):
                view = w[s]["views"].get(k)
                if view:
                    cpp.set_view(True, *view)
                    py.set_view(True, *view)
                a, want = cpp.process(x, K.FREQ, w[s]["rates"][k]), py.process_input(x, K.FREQ, w[s]["rates"][k])
                assert cpp.desired_input_size() == py.desired_input_size, (F, s, k)
                assert (a is None) == (want is None), (F, s, k)
                if a is None:
                    continue
                nout += 1
                assert _same(a[0], want[0]), (F, s, k)
                assert _same(np.float64([a[1], a[2]]), np.float64([want[1], want[2]])), (F, s, k)
                assert a[3] is None and want[3] is None
        finally:
            cpp.close()
    assert nout == 13 + 14 + 13 + 14
