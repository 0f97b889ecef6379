"""GPU: the one argument-count refusal of the MEX gateway that its command table cannot make, because it depends on a value:
'elbo' with separate_K set sizes I_sk by numel(gp.post), its 13th argument.  A handler runs behind the context, so unlike the
table's refusals (tests/test_mex_gateway_compiles.py, no device needed) this one is only reached on a machine with a device."""
import numpy as np
import pytest

from tests._mex import MexError
from tests.test_gpu_mex import make, vp_struct

pytestmark = pytest.mark.gpu


def test_elbo_with_separate_K_needs_numel_gp_post():
    from tests import _mex

    m = _mex.mex()
    m.call(0, "open", 0)
    _, _, vp, theta = make()
    args = [np.uint64(0), theta.reshape(-1, 1), vp_struct(vp), 0, 0, 0, 1, 0, None, None, 7]      # entropy only; up to the seed
    with pytest.raises(MexError) as e:
        m.call(8, "elbo", *args)
    assert e.value.identifier == "vbmc_hip:usage" and "13th argument" in e.value.message, e.value.message
    (F,) = m.call(1, "elbo", *args[:6], 0, *args[7:])                                               # without separate_K the same call is whole
    assert F.shape == (1, 1) and np.isfinite(F[0, 0])
    assert m.live_arrays() == 0
