"""lddl_infill_params (include/lddl_amd.h): the Poisson length law and the start
probability of text infilling, on the host: no GPU, no ctx."""
import ctypes
import math

import numpy as np
import pytest

import infill_model as im

EINVAL = -1


@pytest.mark.parametrize('L,lam,ratio', [(10, 3.0, 0.3), (1, 1.0, 0.5), (16, 6.0, 0.9), (16, 0.01, 0.3), (5, 40.0, 0.15)])
def test_law_and_coverage(L, lam, ratio):
  q, cdf = im.params(L, lam, ratio)
  # the closed form in extended precision, rounded once: the library may be 1 ulp off it
  l = np.arange(1, L + 1)
  w = np.longdouble(lam) ** l / np.asarray([math.factorial(int(x)) for x in l], np.longdouble)
  want = np.ones(16)
  want[:L - 1] = (np.cumsum(w) / w.sum())[:L - 1].astype(np.float64)
  assert (np.abs(cdf - want) <= np.spacing(want)).all() and (cdf[L - 1:] == 1.0).all()
  # The last bisection interval is <= 2^-52 wide and the coverage's slope in q is <= sum S_t <= 16: the residual
  # is <= 2^-48 plus rounding
  S = np.concatenate([[1.0], 1.0 - cdf[:L - 1]])
  assert abs(1.0 - np.prod(1.0 - q * S) - ratio) <= 1e-12
  assert 0.0 < q <= ratio and im.params(L, lam, 0.0)[0] == 0.0 and im.params(L, lam, 1.0)[0] == 1.0


@pytest.mark.parametrize('L,lam,ratio', [(0, 3.0, 0.3), (17, 3.0, 0.3), (10, 0.0, 0.3), (10, -1.0, 0.3),
                                         (10, float('inf'), 0.3), (10, float('nan'), 0.3), (10, 3.0, -0.1),
                                         (10, 3.0, 1.5), (10, 3.0, float('nan'))])
def test_refused_arguments(L, lam, ratio):
  from lddl_amd import _lib
  q, cdf = ctypes.c_double(), (ctypes.c_double * 16)()
  assert _lib.lib().lddl_infill_params(L, lam, ratio, ctypes.byref(q), cdf) == EINVAL
  assert _lib.lib().lddl_infill_params(10, 3.0, 0.3, None, cdf) == EINVAL  # a NULL output
  assert _lib.lib().lddl_infill_params(10, 3.0, 0.3, ctypes.byref(q), None) == EINVAL
