"""wtamd_EnergyIntegrator and wtamd_EnergySpectrum of the product over array children, an overlapping child, popping children and
a MeanReduction of two tracks (drained in blocks), with the device door and again with WTAMD_NO_DEVICE_ENERGY=1: the recorded
exact values within the door's bound, the spectrum of k wavelengths equal to k integrators bit for bit
(tests/energy_dropin.py, which tests/test_energy_dropin_host.py runs over the emulated drop-in library)."""
import ctypes as C
import os

import numpy as np
import pytest

import energy_dropin
import energy_model as M

pytestmark = pytest.mark.gpu


def test_dropin():
    from wiggletools_amd import _lib

    def setenv(k, v):
        os.environ[k] = v

    try:
        energy_dropin.check_dropin(energy_dropin.DropIn(_lib.LIB_PATH), M.fixtures(), setenv)
    finally:
        os.environ.pop("WTAMD_NO_DEVICE_ENERGY", None)


def test_a_mean_reduction_of_two_tracks_is_drained_in_blocks():
    """The mean of a track and itself is the track (values that are multiples of 1/8: exact in float32 and under the mean)."""
    from wiggletools_amd import _lib
    D = energy_dropin.DropIn(_lib.LIB_PATH)
    c = [c for c in M.fixtures() if not c["seek"] and len(c["chroms"]) == 3 and energy_dropin._f32_exact(M.fixture_child(c)[1])
         and not np.isnan(M.fixture_exact(c)).any()][0]
    names, child = M.fixture_child(c)[0], M.fixture_lists(c)        # (the union of the fixture's child: sorted and disjoint)
    lam = M.fixture_wavelengths(c)
    kids = (C.c_void_p * 2)(D.bulk_child(names, child, False), D.bulk_child(names, child, False))
    D.keep.append(kids)
    red = D.L.MeanReduction(D.L.newMultiplexer(kids, 2, b"\x00"))
    got = D.spectrum(red, lam)
    L = M.fixture_lists(c)
    # (the reducer may cut runs or serve the gaps between them at the default 0, which adds nothing to S: 3 n + 3 runs cover both)
    M.check_close(got, M.fixture_exact(c), 3 * len(L.s) + 3, M._num(c["S"]), c["name"])


def test_python_dropin_energy():
    from wiggletools_amd import dropin
    c = [c for c in M.fixtures() if not c["overlaps"] and not c["seek"] and energy_dropin._f32_exact(M.fixture_child(c)[1]) and not np.isnan(M.fixture_exact(c)).any()][0]
    names, child, _ = M.fixture_child(c)
    lam = M.fixture_wavelengths(c)
    s, f, v = child.s, child.f, np.ascontiguousarray(child.v, np.float32)

    def kid():
        return dropin.array_reader(names, child.seg, s.ctypes.data, f.ctypes.data, v.ctypes.data)

    reim, e = dropin.energy_spectrum(kid(), lam)
    M.check_close(reim, M.fixture_exact(c), len(child.s), M._num(c["S"]), c["name"])
    wi = dropin.energy_integrator(kid(), lam[3])
    assert np.isnan(dropin.energy_result(wi)[0])
    dropin.drain_pops(wi)
    res, re_, im_ = dropin.energy_result(wi)
    assert M.same_bits([re_, im_], reim[3]) and res == e[3]
