"""The bundle adjustments' three solver paths under both entries on the device (MI355X): cases and checks in ba_solver_cases.py.  What differs from the emulator here is
the code these shapes are chosen for: the wave-level diagonal tile (sgx_chol_diag_wave_body, k_chol_diag_wave), the MFMA tile products of k_chol_env_factor and
k_chol_update_wide, and the device builder of the Schur job list."""
import pytest
import ba_solver_cases as sc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', sc.GLOBAL)
def test_global_ba_matches_oracle_gpu(gpulib_taps, oracle, name):
    sc.check_global(gpulib_taps, oracle, name)


@pytest.mark.parametrize('name', sc.LOCAL_ORACLE)
def test_local_ba_matches_oracle_gpu(gpulib_taps, oracle, name):
    sc.check_local(gpulib_taps, oracle, name)


@pytest.mark.parametrize('name,entry', sc.INIT)
def test_initialisation_independence_gpu(gpulib_taps, oracle, name, entry):
    sc.check_init(gpulib_taps, oracle, name, entry)


@pytest.mark.parametrize('name,entry', sc.HISTORY)
def test_history_independence_gpu(gpulib, oracle, name, entry):
    """the product library: no tap forces a solver there, so below 1024 unknowns X runs on the dense path and only auto-172 on the envelope"""
    sc.check_history(gpulib, oracle, name, entry)


@pytest.mark.parametrize('name,entry', [(n, e) for n, e in sc.HISTORY if sc.CASES[n]['solver'] == 2])
def test_history_independence_forced_envelope_gpu(gpulib_taps, oracle, name, entry):
    """the tap build, for the X whose envelope has to be forced: the plan is asserted on every run of X"""
    sc.check_history(gpulib_taps, oracle, name, entry)
