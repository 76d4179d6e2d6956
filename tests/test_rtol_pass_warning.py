"""CPU only: the Python layer warns once per process when an early exit (rtol > 0) that did not ask for the pass-by-pass path lands on it all the
same (images up to 128 columns wide) -- that path synchronises the stream after every pass; exit_path='passes' stays silent."""
import warnings

import pytest

from lmc_atomi_amd import proximal as P


@pytest.mark.parametrize("W,tv_rtol,ncvx_rtol,exit_path,want", [
    (96, 1e-4, 0.0, 0, True), (128, 0.0, 1e-4, 0, True),          # narrow image, TV prior / ME-TV inner prox
    (96, 1e-4, 0.0, 1, False),                                    # asked for: silent
    (96, 0.0, 0.0, 0, False),                                     # fixed count
    (129, 1e-4, 1e-4, 0, False), (877, 1e-4, 0.0, 0, False), (1544, 0.0, 1e-4, 0, False),      # decided on the device
])
def test_which_problems_land_on_the_pass_by_pass_path(W, tv_rtol, ncvx_rtol, exit_path, want):
    assert P._exit_lands_on_passes(W, tv_rtol, ncvx_rtol, exit_path) is want


def test_the_warning_is_raised_once_per_process(monkeypatch):
    monkeypatch.setattr(P, "_warned_pass_by_pass", False)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        P._warn_pass_by_pass(96)
        P._warn_pass_by_pass(64)
    assert len(rec) == 1 and rec[0].category is RuntimeWarning
    assert "synchronises" in str(rec[0].message) and "96" in str(rec[0].message)
