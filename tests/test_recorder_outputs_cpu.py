"""Each recorder evaluator's outputs, stated once (history.EVALUATORS): the table against the declarations of
include/jsim_mpc.h and the binding's argtypes, the Recorder's home, and Recorder._outputs on a stand-in recorder without a device."""
import os
import re
import types

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the outputs an entry point has beside its per-tick ones: they stay explicit in the Recorder's methods
EXPLICIT = {"reasons": ("carry", "first"), "cutoffs": ("carry",)}
EVALUATORS = ("reasons", "conflicts", "gaps", "static", "tracking", "headway", "cutoffs")


def declaration(pkg, entry):
    """The parameters of an entry point's declaration in the header, in order: (name, whether the call may write through it)."""
    return [(name, "*" in t and not t.startswith("const ")) for t, name in pkg._header.header().functions[entry].params]


def test_the_table_names_every_evaluator(pkg):
    assert tuple(pkg.history.EVALUATORS) == EVALUATORS
    assert not re.search(r"^\s*(import|from)\s+torch", open(pkg.history.__file__).read(), re.M)     # numpy only


@pytest.mark.parametrize("name", EVALUATORS)
def test_keys_are_the_declarations_trailing_outputs(pkg, name):
    ev = pkg.history.EVALUATORS[name]
    assert ev.entry == "jsim_loop_eval_" + name
    params = declaration(pkg, ev.entry)
    assert params[0] == ("ctx", True) and params[-1] == ("stream", True)
    written = [p for p, out in params[1:-1] if out]
    explicit = EXPLICIT.get(name, ())
    assert [p for p in written if p not in explicit] == list(ev.keys())    # the keys, in the declaration's order
    assert sorted(p for p in written if p in explicit) == sorted(explicit)
    tail = [p for p, _ in params[:-1] if p not in explicit][-len(ev.keys()):]
    assert tail == list(ev.keys())                                         # ... and they are its last parameters
    assert len(getattr(pkg._cabi.load(), ev.entry).argtypes) == len(params)
    assert set(ev.optional) <= set(ev.keys()) and ev.keys(skip=ev.optional) == tuple(k for k in ev.keys() if k not in ev.optional)


def test_the_recorder_lives_in_recorder_py(pkg):
    assert pkg.closed_loop.Recorder is pkg.recorder.Recorder is pkg.Recorder
    assert pkg.closed_loop._register_recorder is pkg.recorder._register_recorder
    assert pkg.closed_loop.vehicle_shape is pkg.vehicle.vehicle_shape and pkg.closed_loop.car_circles is pkg.vehicle.car_circles
    assert pkg.closed_loop.MAX_OBS == pkg.history.MAX_OBS == 8 and pkg.history.EVALUATORS["headway"].optional == ("gap", "lat", "rate")


@pytest.mark.parametrize("n", (0, 2))
def test_outputs_on_a_stand_in_recorder(pkg, n):
    """_outputs gives the table's dtypes and shapes, in its order, with rows to point at when no tick is recorded yet; _rows gives
    the n rows a call wrote."""
    R, B = pkg.recorder.Recorder, 3
    stand_in = types.SimpleNamespace(loop=types.SimpleNamespace(eng=types.SimpleNamespace(B=B, device=torch.device("cpu"))))
    for name, ev in pkg.history.EVALUATORS.items():
        out = R._outputs(stand_in, name, n)
        assert tuple(out) == ev.keys()
        for (k, dt, shape), t in zip(ev.outputs, out.values()):
            assert t.shape == (max(n, 1), B, *shape) and t.numpy().dtype == np.dtype(dt) and t.is_contiguous(), (name, k)
            assert t.data_ptr() != 0, (name, k)
        assert len({t.data_ptr() for t in out.values()}) == len(out)
        rows = R._rows(out, n)
        assert tuple(rows) == ev.keys() and all(rows[k].shape == (n, B, *shape) for k, _, shape in ev.outputs)
        bare = R._outputs(stand_in, name, n, skip=ev.optional)
        assert tuple(bare) == ev.keys() and all((bare[k] is None) == (k in ev.optional) for k in bare)
        assert tuple(R._rows(bare, n)) == ev.keys(skip=ev.optional)
    host = R._host({"a": torch.arange(3), "used": (1, 2)}, ("a",))
    assert isinstance(host["a"], np.ndarray) and host["a"].tolist() == [0, 1, 2] and host["used"] == (1, 2)


def test_the_compiler_fact_is_in_the_design(pkg):
    """DESIGN.md section 5 records what folding the MPC kernels' repeated stages into helpers does to the listing."""
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    five = design[design.index("\n## 5. Kernels"):design.index("\n## 6. ")]
    for text in ("22,845", "54,068", "198", "-DJSIM_KERNEL_TU=13", "__forceinline__", "mpc_step_reg4.inc"):
        assert text in five, text
    assert "\n## 26. " in design and "history.EVALUATORS" in design[design.index("\n## 26. "):]
