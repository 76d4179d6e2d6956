"""CPU only: the Python surface of the anisotropic TV prior -- `TV(..., isotropic=False)` describes itself as LMC_PRIOR_TV_ANISO with the fields of
the TV prox, the default stays the isotropic descriptor, and the options that are not built for it are refused at construction."""
import numpy as np
import pytest

from lmc_atomi_amd import _capi, proximal


def test_anisotropic_descriptor_carries_the_prox_fields():
    d = proximal.TV((24, 40), sigma=0.3, niter=10, isotropic=False).prior_descriptor()
    assert d["prior_kind"] == _capi.PRIOR_TV_ANISO
    assert d["tv_niter"] == 10 and len(d["tv_betas"]) == 10
    assert d["prior_sigma"] == pytest.approx(0.3) and d["tv_step"] == pytest.approx(0.125)
    assert not d["tv_warm"] and d["tv_rtol"] == 0.0


def test_isotropic_descriptor_is_the_old_one():
    old = proximal.TV((24, 40), sigma=0.3, niter=7, momentum="fista").prior_descriptor()
    new = proximal.TV((24, 40), sigma=0.3, niter=7, momentum="fista", isotropic=True).prior_descriptor()
    assert old["prior_kind"] == new["prior_kind"] == _capi.PRIOR_TV_ISO
    assert set(old) == set(new) == {"prior_kind", "prior_sigma", "tv_niter", "tv_step", "tv_betas", "tv_lagged_output", "tv_warm", "tv_rtol", "tv_exit_path"}
    for k in old:
        np.testing.assert_array_equal(old[k], new[k])


def test_early_exit_is_refused_at_construction():
    with pytest.raises(NotImplementedError):
        proximal.TV((24, 40), isotropic=False, rtol=1e-4)
    proximal.TV((24, 40), isotropic=True, rtol=1e-4)


def test_warm_dual_is_refused_at_construction():
    with pytest.raises(NotImplementedError):
        proximal.TV((24, 40), niter=2, isotropic=False, warm=True)
    proximal.TV((24, 40), niter=2, isotropic=True, warm=True)
