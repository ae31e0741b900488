"""What tests/test_energy_dropin_host.py (the emulated drop-in library: the host sweep) and tests/test_energy_dropin_gpu.py (the
product) share: a ctypes driver of wtamd_EnergyIntegrator and wtamd_EnergySpectrum over wtamd_ArrayReader /
wtamd_OverlappingArrayReader children (the bulk path, float32 values) and over a popping child (cover_dropin.DropIn.popping:
the reference's protocol, double values) -- against the recorded fixtures: the exact values within the door's bound, the
reference's recorded values within the reference's."""
import ctypes as C

import numpy as np

import cover_dropin
import energy_model as M


class EnergyView(C.Structure):
    """The head of the integrator's data, laid out as the reference's EnergyData (statistics.c:345-352)."""
    _fields_ = [("res", C.c_double), ("real", C.c_double), ("im", C.c_double), ("wavelength", C.c_int), ("chrom_offset", C.c_int)]


class DropIn(cover_dropin.DropIn):
    def __init__(self, path):
        super().__init__(path)
        L = self.L
        L.wtamd_EnergyIntegrator.restype = C.c_void_p
        L.wtamd_EnergyIntegrator.argtypes = [C.c_void_p, C.c_int]
        L.wtamd_EnergySpectrum.restype = C.c_int
        L.wtamd_EnergySpectrum.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.wtamd_energy_finish.restype = C.c_double
        L.wtamd_energy_finish.argtypes = [C.c_void_p]

    def bulk_child(self, names, lists, overlapping):
        return self.reader(names, lists.seg, lists.s, lists.f, lists.v, overlapping=overlapping)

    def popping_child(self, names, lists, overlapping):
        """A foreign iterator by the reference's protocol over several chromosomes: a WiggleIterator whose pop is a callback,
        double values, stable chromosome names."""
        return self.popping(names, lists.seg, lists.s, lists.f, lists.v, overlapping)

    def integrate(self, child, lam, seek=None):
        """(real, im, res, res before the end) of wtamd_EnergyIntegrator popped to its end; seek = (chrom, start, finish): sought
        right after the constructor, which has served the first chromosome."""
        wi = self.L.wtamd_EnergyIntegrator(child, int(lam))
        w = self.fields(wi)
        early = EnergyView.from_address(w.data).res
        if seek is not None:
            self.seek(wi, *seek)
        while w.done == b"\x00":
            self.L.pop(wi)
        e = EnergyView.from_address(w.data)
        assert w.append == child
        return e.real, e.im, e.res, early

    def spectrum(self, child, lams):
        lam = np.ascontiguousarray(lams, np.int32)
        out = np.full((len(lam), 2), -1.0)
        rc = self.L.wtamd_EnergySpectrum(child, len(lam), lam.ctypes.data, out.ctypes.data)
        assert rc == 0
        return out


def _f32_exact(L):
    return np.array_equal(L.v.astype(np.float32).astype(np.float64), L.v, equal_nan=True)


def check_dropin(D, fixtures, setenv=None):
    """The checks both backends share.  setenv(name, value): given by the product's test, which reads every case with the
    device door and again with WTAMD_NO_DEVICE_ENERGY=1."""
    seen = {"bulk": 0, "pops": 0, "seek": 0, "overlaps": 0, "nan": 0}
    for c in fixtures:
        names, child, over = M.fixture_child(c)
        lists = M.fixture_lists(c)
        lams, star, ref = M.fixture_wavelengths(c), M.fixture_exact(c), M.fixture_reference(c)
        n, S = len(lists.s), M._num(c["S"])
        P = max([abs(b + int(x)) for g, b in enumerate(M.bases(lists)[0]) for x in list(lists.s[lists.seg[g]:lists.seg[g + 1]]) + list(lists.f[lists.seg[g]:lists.seg[g + 1]])] + [0])
        B = int((lists.f.astype(np.int64) - lists.s).sum())
        sk = c.get("seek")
        seek = (sk["chrom"], sk["start"], sk["finish"]) if sk else None
        bulk_ok = _f32_exact(child)                         # (the array readers hold float32 values)
        if seek is not None and not bulk_ok:
            continue                                        # (the popping child does not seek)
        make = (lambda: D.bulk_child(names, child, over)) if bulk_ok else (lambda: D.popping_child(names, child, over))
        for no_device in (("0", "1") if setenv else ("0",)):
            if setenv:
                setenv("WTAMD_NO_DEVICE_ENERGY", no_device)
            got = np.array([D.integrate(make(), lam, seek) for lam in lams])
            assert np.isnan(got[:, 3]).all(), (c["name"], "res is NaN before the end")
            M.check_close(got[:, :2], star, n, S, (c["name"], no_device))
            if not np.isnan(star).any():
                assert M.same_bits(got[:, 2], M.energy(got[:, :2])), c["name"]
                # the reference's recorded sums: within the door's bound plus the reference's own
                for k, lam in enumerate(lams):
                    t = M.door_bound(n, S) + 2.0 ** -53 * S * (16.0 * P / lam + B + 8)
                    assert (np.abs(got[k, :2] - ref[k, :2]) <= t).all(), (c["name"], lam, got[k], ref[k])
            else:
                assert np.isnan(got[:, 2]).all()
            if seek is None:                                # one drain, every wavelength: the integrators' bits
                assert M.same_bits(D.spectrum(make(), lams), got[:, :2]), (c["name"], "spectrum", no_device)
        seen["bulk" if bulk_ok else "pops"] += 1
        seen["seek"] += int(seek is not None)
        seen["overlaps"] += int(over)
        seen["nan"] += int(np.isnan(star).any())
    assert min(seen.values()) >= 1, seen
    # a wavelength the door refuses: 0 gives NaN; a negative one is the reference's expression, cos(-x) = cos(x), sin(-x) = -sin(x)
    names, child, over = M.fixture_child(fixtures[0])
    assert _f32_exact(child) and not over
    re0, im0, res0, _ = D.integrate(D.bulk_child(names, child, over), 0)
    assert np.isnan(res0)
    pos = D.integrate(D.bulk_child(names, child, over), 7)
    neg = D.integrate(D.bulk_child(names, child, over), -7)
    t = M.door_bound(len(child.s), M._num(fixtures[0]["S"])) + 2.0 ** -53 * M._num(fixtures[0]["S"]) * (16.0 * 2 ** 17 / 7 + 2 * 10 ** 4 + 8)
    assert abs(neg[0] - pos[0]) <= t and abs(neg[1] + pos[1]) <= t, (neg, pos)
    mixed = D.spectrum(D.bulk_child(names, child, over), [7, 0, -7])
    assert M.same_bits(mixed[0], pos[:2]) and np.isnan(mixed[1]).all() and M.same_bits(mixed[2], neg[:2])
    assert D.L.wtamd_energy_finish(np.array([3.0, 4.0]).ctypes.data) == 25.0
