"""The ego sets of tests/test_gpu_j_register_set.py exercise what that test is about, shown on the CPU oracle alone: in the oracle's
closed loop (oracle_py.closed_loop) of every horizon's set some ego needs more than 2T active-set iterations in one tick.  An
iteration ends in an add or in a drop and the working set holds at most the 2T variables, so such a solve has dropped a row at
least once -- and added many: both paths that carry J's row through the bottom of the step-2 loop are taken."""
import pytest

import j_register_set_cases as C


@pytest.mark.parametrize("T", (13, 20, 30, 40))
def test_oracle_closed_loop_has_drops_and_a_long_solve(pkg, oracle, T):
    routes = C.synthetic_routes(pkg)
    batch = C.ego_set(pkg, routes, T)
    ticks = C.TICKS1 if T <= 20 else C.TICKS4
    assert batch.x0.shape[0] == (C.B1 if T <= 20 else C.B4)
    it = C.oracle_iterations(oracle, pkg, routes, batch, T, ticks)
    print(f"T = {T}: oracle iterations per tick and ego\n{it}")
    assert it.max() > 2 * T                   # a long solve, which has at least (it.max() - 2T + 1) // 2 drops
    assert (it > 0).sum() > it.size // 2      # and most solves add rows at all
