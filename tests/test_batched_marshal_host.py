"""CPU: what every wrapper of ``batched`` hands to libmpcqp -- the entry point,
each argument, the tensors it allocates or converts, the structure it returns
and every ValueError with its text -- equals what the parent commit of the
marshalling refactor handed over, case by case (tests/_batched_record.py; the
record of the parent is tests/golden/batched_calls.json, written from a
checkout of that commit and never from the tree under test)."""
import json
import os
import re

import pytest

import _batched_record as rec
from model_predictive_control_amd import batched

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

with open(os.path.join(ROOT, "tests", "golden", "batched_calls.json")) as _fh:
    GOLDEN = json.load(_fh)


def test_case_table_and_record_agree():
    assert re.fullmatch(r"[0-9a-f]{40}", GOLDEN["parent"])
    assert set(GOLDEN["cases"]) == set(rec.CASES), set(GOLDEN["cases"]) ^ set(rec.CASES)
    assert len(rec.CASES) >= 300


@pytest.mark.parametrize("name", sorted(set(rec.CASES) | set(GOLDEN["cases"])))
def test_same_calls_as_parent(name):
    assert name in rec.CASES and name in GOLDEN["cases"], name
    got, want = rec.run_case(rec.CASES[name]), GOLDEN["cases"][name]
    assert got.get("error") == want.get("error")
    assert got["calls"] == want["calls"]
    assert got == want


def test_seams_restored_and_public_names_kept():
    for k, v in rec._ORIG.items():
        assert getattr(batched, k) is v
    for k in ("_ptr", "_stream", "_bike_params", "_weight_r", "_bound_pair", "_lib", "_dev",
              "_workspace", "_WS"):
        assert hasattr(batched, k), k
    assert sorted(batched.__all__) == sorted([
        "condense", "solve_box", "solve_box_vjp", "mpc_box", "mpc_box_loop", "mpc_box_loop_vjp",
        "mpc_poly_loop", "tracking_terms", "mpc_qp", "mpc_ipm", "solve_poly", "solve_qp", "sweep",
        "riccati", "gemv", "rollout", "bicycle_rti", "bicycle_linearise", "bicycle_hessian",
        "bicycle_sqp_step", "pack_lower", "unpack_lower", "status_code", "status_iters",
        "workspace_bytes"])
