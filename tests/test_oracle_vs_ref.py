"""Pins the C restatement (oracle/edm_oracle.c) against the REAL reference: what the reference build
(oracle/_ref/libedm_ref.so, oracle/Makefile) observed on the cases of tests/oracle_ref_cases.py is stored in
tests/golden/vsref_<kind>.npz by oracle/gen_golden.py; each test runs the same case on the oracle.

Every comparison is bit-exact on doubles and exact on integers / file bytes (files by SHA-256).
"""
import numpy as np
import pytest

import oracle_ref_cases as RC
from conftest import FIXTURES, GOLDEN

_GOLDEN = {}


def golden(kind):
    if kind not in _GOLDEN:
        _GOLDEN[kind] = np.load(RC.golden_path(GOLDEN, kind), allow_pickle=False)
    return _GOLDEN[kind]


@pytest.mark.parametrize("case", RC.GRID_CASES)
@pytest.mark.parametrize("deriv,interp", RC.GRID_MODES)
def test_grid_geometry_index_lookup(oracle_lib, case, deriv, interp):
    i = RC.GRID_CASES.index(case)
    obs = RC.run_grid(oracle_lib, i, deriv, interp)
    assert np.array_equal(obs["multi2one"], obs["one2multi_at"])
    assert not np.asarray(obs["values_after_clear"]).any()
    RC.assert_matches(golden("grid"), RC.grid_case_id(i, deriv, interp), obs)


@pytest.mark.parametrize("name,dim", RC.READ_CASES)
def test_grid_read_write(oracle_lib, workdir, name, dim):
    obs = RC.run_grid_read_write(oracle_lib, FIXTURES, workdir, name, dim)
    assert obs["has_deriv"] == 1
    RC.assert_matches(golden("grid_files"), name, obs)


def test_grid_add_grid(oracle_lib):
    RC.assert_matches(golden("grid_files"), "add_grid", RC.run_grid_add_grid(oracle_lib, FIXTURES))


@pytest.mark.parametrize("c", RC.GAUSS_CASES)
def test_gauss_setup_tables_remap(oracle_lib, c):
    i = RC.GAUSS_CASES.index(c)
    RC.assert_matches(golden("gauss_setup"), "case%d" % i, RC.run_gauss_setup(oracle_lib, i))


@pytest.mark.parametrize("c", RC.GAUSS_CASES)
def test_gauss_add_value_and_lookup(oracle_lib, c):
    i = RC.GAUSS_CASES.index(c)
    RC.assert_matches(golden("gauss_lookup"), "case%d" % i, RC.run_gauss_add_lookup(oracle_lib, i))


@pytest.mark.parametrize("name", sorted(RC.BIAS_CFGS))
def test_bias_controller_sequences(oracle_lib, workdir, name):
    obs = RC.run_bias(oracle_lib, name, workdir)
    RC.assert_matches(golden("bias"), name, obs)
    if name == "c1d_limit":
        assert max(v[1] for v in obs["ov"]) > 0  # the overflow buffer was exercised


def test_config_reader(oracle_lib, workdir):
    obs = RC.run_config_reader(oracle_lib, FIXTURES, workdir)
    RC.assert_matches(golden("bias"), "config_reader", obs)
    v = obs["values"]
    assert v[0] == 2 and v[1] == 0 and v[-4:] == [2.0, 1.0, 1.0, 1.0]


# ---------------------------------------------------------------------------------
# the pair fix's own loop order (lammps/fix_edm_pair.cpp:173-247)
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", RC.PAIR_FIX_SEEDS)
def test_pair_fix_order(oracle_lib, workdir, seed):
    RC.assert_matches(golden("bias"), "pair_fix_seed%d" % seed, RC.run_pair_fix(oracle_lib, workdir, seed))
