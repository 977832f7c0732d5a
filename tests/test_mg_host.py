"""The multigrid-preconditioned solve's host side (no GPU needed): the structs behind
``ptv_abi_sizes13``, the exported names, the parameter dict and the refusals that are decided before
any device call."""
import numpy as np
import pytest

from ptv_interpolation_amd import _lib, physics, velocity_analysis


def test_abi_sizes13_match_ctypes():
    c, py = _lib.abi_sizes13()
    assert c == py


def test_symbols_exported_and_version_unchanged():
    for name in ("ptv_abi_sizes13", "ptv_poisson_mg_apply", "ptv_poisson_mg_apply_dev", "ptv_poisson_solve_mg",
                 "ptv_poisson_solve_mg_dev", "ptv_pressure_recover_mg", "ptv_pressure_recover_mg_dev"):
        assert hasattr(_lib.lib(), name) and name in _lib.EXPORTS
    assert _lib.lib().ptv_version() == 11


def test_parameter_dict():
    prm = _lib.mg_params({"nu": 3, "omega": 0.8})
    assert (prm.max_levels, prm.nu, prm.coarse_sweeps, prm.omega) == (0, 3, 0, 0.8)
    assert _lib.mg_params(None).nu == 0
    with pytest.raises(ValueError):
        _lib.mg_params({"sweeps": 2})


def test_refusals_come_before_any_device_work():
    shape = (4, 5, 6)
    mask = np.ones(shape, bool)
    rhs = np.zeros(shape)
    with pytest.raises(NotImplementedError, match="LSQR"):
        physics.solve_poisson(rhs, mask, 1.0, 1.0, 1.0, preconditioner="multigrid")
    with pytest.raises(ValueError):
        physics.solve_poisson(rhs, mask, 1.0, 1.0, 1.0, dirichlet_mask=mask, preconditioner="ilu")
    with pytest.raises(ValueError):
        physics.solve_poisson(rhs, mask, 1.0, 1.0, 1.0, dirichlet_mask=mask, multigrid={"nu": 1})
    with pytest.raises(NotImplementedError, match="LSQR"):
        velocity_analysis.recover_pressure(rhs, rhs, rhs, 1.0, 1.0, 1.0, 1e-3, 0, mask, anchor="none",
                                           preconditioner="multigrid")
    with pytest.raises(ValueError):
        velocity_analysis.compute_pressure_field(rhs, rhs, rhs, 1.0, 1.0, 1.0, 1e-3, 0, mask,
                                                 preconditioner="multigrid", multigrid={"levels": 2})
