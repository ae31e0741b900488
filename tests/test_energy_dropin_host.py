"""wtamd_EnergyIntegrator and wtamd_EnergySpectrum of the emulated drop-in library (tests/emu/build.py: csrc/wt_iter_abi.cpp without
the HIP units, so the host sweep of csrc/wt_energy.h) over bulk, overlapping and popping children, a seek in the middle
included: the recorded exact values within the door's bound, the reference's recorded sums within its own, a wavelength of 0
giving NaN (tests/energy_dropin.py, which tests/test_energy_dropin_gpu.py runs over the product)."""
import energy_dropin
import energy_model as M
from emu import build as emu_build


def test_the_dropin_energy_on_the_host_sweep():
    energy_dropin.check_dropin(energy_dropin.DropIn(emu_build.build_dropin()), M.fixtures())
