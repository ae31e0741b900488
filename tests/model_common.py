"""Helpers the units' models (tests/*_model.py) had word for word in common; each model re-exports the ones it uses under their
old names.  Comparisons that differ between models (cover_model.same_bits also compares NaN payloads; window_model.py and
exact.py have their own rules) stay where they are."""
import ctypes as C

import numpy as np


def _p(a):
    return C.c_void_p(a.ctypes.data)


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def same_bits(a, b):
    """Equal as doubles bit for bit, any NaN equal to any NaN (hist_model, energy_model)."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def _num(x):
    """A recorded number: None is NaN, a string is float.hex()."""
    return float("nan") if x is None else float.fromhex(x) if isinstance(x, str) else float(x)
