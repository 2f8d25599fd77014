"""K0 / K5 fit queries over a grid of shapes vs the committed table (no GPU).

tests/generic_fit_table.json holds what the parent commit's library answered, when each of K5's four objects (ELU(1), act, pre, tableau)
had fit functions of its own meaning and the pre object exported a second fit query; it was written by
profiles/scripts/generic_fit_table.py, which also defines the grid and the queries.  K5's fit and LDS-layout functions now take `pre` as a
run-time argument and generic_bwd_fits answers for every build from one object: every answer -- for the DAE backward, K5's mode -- has to
be the one it was.  The four forward rows are all '1' (K0 fits every shape of the grid): they pin the entry points, not K0's fit."""
import importlib.util
import json
import os

import pytest

from py_psnode_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("generic_fit_table", os.path.join(HERE, "..", "profiles", "scripts", "generic_fit_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(HERE, "generic_fit_table.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def answers(gen):
    return gen.answers(_lib)


def test_table_is_the_scripts_grid(gen, table):
    assert tuple(table["depths"]) == gen.DEPTHS and tuple(table["hidden"]) == gen.HIDDEN
    assert tuple(table["ode_x"]) == gen.ODE_X and tuple(table["ode_z"]) == gen.ODE_Z
    assert tuple(tuple(d) for d in table["dae_dims"]) == gen.DAE_DIMS
    assert set(table["answers"]) == set(gen.ODE_QUERIES + gen.DAE_QUERIES) and len(table["answers"]) == 12
    for q in gen.ODE_QUERIES:
        assert len(table["answers"][q]) == len(gen.ode_shapes())
    for q in gen.DAE_QUERIES:
        assert len(table["answers"][q]) == len(gen.dae_shapes())


def test_table_is_not_constant(gen, table):
    """Every backward query is answered both ways somewhere, and the grid holds the boundary test_activations_pre_host.py pins: hidden
    160 x 3, z_dim 2 fits the pre build up to x_dim 24 and not at 32, where Tanh still fits."""
    for q, s in table["answers"].items():
        if "backward" in q:
            assert "0" in s and s.strip("0"), q
    assert set(table["answers"]["dae_backward"]) == {"0", "1", "2"}
    shapes = gen.ode_shapes()
    inside, outside = shapes.index((4, 160, 24, 2)), shapes.index((4, 160, 32, 2))
    a = table["answers"]
    assert a["ode_backward_act_silu"][inside] == "1" and a["ode_backward_act_silu"][outside] == "0"
    assert a["ode_backward_rk_heun2"][inside] == "1" and a["ode_backward_rk_heun2"][outside] == "0"
    assert a["ode_backward_act_tanh"][outside] == "1" and a["ode_backward"][outside] == "1"


def test_every_answer_is_the_tables(gen, table, answers):
    for q in gen.ODE_QUERIES + gen.DAE_QUERIES:
        shapes = gen.ode_shapes() if q in gen.ODE_QUERIES else gen.dae_shapes()
        diff = [(shapes[k], table["answers"][q][k], answers[q][k]) for k in range(len(shapes)) if table["answers"][q][k] != answers[q][k]]
        assert not diff, f"{q}: {len(diff)} answers differ from the table (shape, table, library), first {diff[:5]}"
