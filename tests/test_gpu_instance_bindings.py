"""The binding record of a handle (ilqg_problem::bindings, csrc/ilqg_instances.hpp): every table bound on a handle is bound
for the same batch.  A bind of a second table for another batch, and a call that would read a bound table on another
number of instances, are refused with ILQG_ERR_INVALID and the texts below — literals, not built from the library's table
of words.  Batches of 4 against 3: the smallest at which a mismatch exists.  No solves.

The scene is two_car_scene (tests/test_instance_time_nominals.py), the one
test_values_routes_and_time_nominals_bound_together_in_every_order binds all three tables on: its second lane carries no
route-progress term, so it may vary per instance.  (mixed_route_scene's only polyline carries one: declaring it is
refused, so that scene cannot hold a route table.)"""
import itertools

import numpy as np
import pytest

from ilqgames_amd import abi
from test_instance_time_nominals import two_car_scene

pytestmark = pytest.mark.gpu

BOUND, OTHER = 4, 3

BIND_REFUSALS = {
    ("values", "routes"): "instance routes: per-instance parameter values are bound for a batch of 4, these routes are for 3",
    ("values", "nominals"): "instance time nominals: per-instance parameter values are bound for a batch of 4, these nominals "
                            "are for 3",
    ("routes", "values"): "instance parameter values: per-instance routes are bound for a batch of 4, these values are for 3",
    ("routes", "nominals"): "instance time nominals: per-instance routes are bound for a batch of 4, these nominals are for 3",
    ("nominals", "values"): "instance parameter values: per-instance time nominals are bound for a batch of 4, these values "
                            "are for 3",
    ("nominals", "routes"): "instance routes: per-instance time nominals are bound for a batch of 4, these routes are for 3",
}
CALL_REFUSALS = {
    "values": "per-instance parameter values are bound for a batch of 4, this call has 3 instances",
    "routes": "per-instance routes are bound for a batch of 4, this call has 3 instances",
    "nominals": "per-instance time nominals are bound for a batch of 4, this call has 3 instances",
}


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from ilqgames_amd import hip as h
    name, _ = h.device_info()
    assert "gfx950" in name, name
    return h


def _declared_problem(hip, subsystem_column=False):
    """-> (the problem with a value column and lane 2 declared, table -> (batch -> bind it / None -> unbind it))."""
    spec = two_car_scene()
    prob = hip.Problem(spec, abi.F64)
    prob.declare_instance_params([(2, "value")])  # player 1's nominal speed
    if subsystem_column:
        prob.declare_instance_subsystem_params([1])  # player 2's wheelbase
    prob.declare_instance_routes([1])
    columns = 2 if subsystem_column else 1
    tables = len(prob.time_nominal_terms())
    lane = np.array([(-20.0, -3.0), (20.0, -3.0)], dtype=np.float32)
    baked = hip.time_nominal_table(spec, abi.F64)
    binds = {"values": lambda B: prob.bind_instance_values(None if B is None else np.full((B, columns), 4.0, np.float32)),
             "routes": lambda B: prob.bind_instance_routes(None if B is None else np.tile(lane, (B, 1, 1))),
             "nominals": lambda B: prob.bind_instance_time_nominals(None if B is None else np.tile(baked, (B, 1, 1, 1)))}
    assert baked.shape == (tables, spec.T, 2)
    return prob, binds


def _refused(hip, call, text):
    with pytest.raises(hip.IlqgError) as e:
        call()
    assert e.value.status == abi.ERR_INVALID
    assert str(e.value) == "ilqg status %d: %s" % (abi.ERR_INVALID, text)


@pytest.mark.parametrize("first,second", list(itertools.permutations(("values", "routes", "nominals"), 2)))
def test_bind_for_another_batch_is_refused(hip, first, second):
    prob, binds = _declared_problem(hip)
    binds[first](BOUND)
    _refused(hip, lambda: binds[second](OTHER), BIND_REFUSALS[(first, second)])
    binds[second](BOUND)  # the same batch is accepted, and the refusal left the first table bound
    _refused(hip, lambda: binds[second](OTHER), BIND_REFUSALS[(first, second)])
    binds[first](None)
    binds[second](OTHER)  # alone, a table may be bound again for any batch


@pytest.mark.parametrize("table,subsystem_column", [("values", False), ("values", True), ("routes", False),
                                                    ("nominals", False)])
def test_entry_points_with_one_table_bound(hip, table, subsystem_column):
    """A cost-evaluating call on another batch is refused; one that only integrates reads no segment and no nominal, and
    of the value table only a subsystem column."""
    prob, binds = _declared_problem(hip, subsystem_column)
    spec = prob.spec
    x0 = np.tile(np.asarray(spec.x0, dtype=np.float64), (OTHER, 1))
    xs = np.tile(x0[:, None, :], (1, spec.T, 1))
    us = np.zeros((OTHER, spec.T, spec.m))
    P = np.zeros((OTHER, spec.T, spec.m * spec.n))

    def total_costs():
        return prob.total_costs(xs, us)

    def rollout():
        return prob.rollout(x0, xs, us, P, us)

    binds[table](BOUND)
    _refused(hip, total_costs, CALL_REFUSALS[table])
    if table == "values" and subsystem_column:
        _refused(hip, rollout, CALL_REFUSALS[table])
    else:
        rollout()
    binds[table](None)
    total_costs()
    rollout()
