"""CPU: the stage-wise interior point (csrc/ipm_lane.hpp on the component
algebra and iteration control of csrc/ipm_step.hpp) compiled for the host by
tools/ipm_host.cpp, against the golden minimisers and the oracle, and its
decision ladder driven into every exit.

Built without contraction (-ffp-contract=off), so the iterates are plain IEEE
arithmetic: the status words (code, iteration count, polished bit) of the two
full runs were recorded once with the headers before ipm_step.hpp existed
(tests/golden/ipm_host_status.npz) and are asserted exactly.  Figures of that
build: (2,1) golden max|z - z*| 2.3e-13 with 5 to 17 iterations; (4,2) batch
5e-14 in z, 5e-13 relative in y, 6 to 9 iterations."""
import numpy as np
import pytest

import _ipm_cases as ic
from model_predictive_control_amd._native import (STATUS_MAXITER, STATUS_NONFINITE,
                                                  STATUS_NOT_CONVEX, STATUS_OPTIMAL,
                                                  STATUS_POLISHED)

TOL = 1e-9
TOL_Y = 1e-7  # relative to 1 + max|y|


@pytest.fixture(scope="module")
def runs(tmp_path_factory, golden):
    lib = ic.build_host(tmp_path_factory.mktemp("ipm_host"))
    if lib is None:
        pytest.skip("no g++")
    return ic.host_runs(lib, golden)


def _code(st):
    return st & 0xFF


def _iters(st):
    return (st >> 8) & 0xFFFF


def test_host_cfg2_golden(runs, golden):
    """(2, 1): the 64 golden BVLS minimisers of config 2."""
    g, r = golden("boxqp_cfg2.npz"), runs["cfg2"]
    assert (_code(r["status"]) == STATUS_OPTIMAL).all()
    assert ((r["status"] & STATUS_POLISHED) != 0).all()
    err = float(np.abs(r["z"] - g["z"]).max())
    print("cfg2 max|z - z*|", err, "iterations", _iters(r["status"]).min(),
          _iters(r["status"]).max())
    assert err < TOL, err
    assert (r["status"] == golden("ipm_host_status.npz")["cfg2"]).all()


def test_host_tv_batch_vs_oracle(runs, golden):
    """(4, 2), every stage matrix its own, N = 12: z, X and the state
    multipliers against the condensed QP solved by the oracle's active set."""
    o, r = ic.tv_oracle(), runs["tv"]
    # what makes the batch a test: every instance solved (solve_oracle raises
    # otherwise), each with an active set, state and input rows both active
    assert len(o["act_x"]) == ic.BATCH
    assert min(x + u for x, u in zip(o["act_x"], o["act_u"])) >= 5
    assert sum(o["act_x"]) > 0 and sum(o["act_u"]) > 0
    assert (_code(r["status"]) == STATUS_OPTIMAL).all()
    assert ((r["status"] & STATUS_POLISHED) != 0).all()
    ez = float(np.abs(r["z"] - o["z"]).max())
    ex = float(np.abs(r["X"] - o["X"]).max())
    ey = float((np.abs(r["y"] - o["y"]).max(1) / (1.0 + np.abs(o["y"]).max(1))).max())
    print("tv z", ez, "X", ex, "y", ey, "iterations", _iters(r["status"]).min(),
          _iters(r["status"]).max())
    assert ez < TOL, ez
    assert ex < TOL, ex
    assert ey < TOL_Y, ey
    assert (r["status"] == golden("ipm_host_status.npz")["tv"]).all()


def test_host_ladder_maxiter(runs):
    st = runs["maxiter"]["status"]
    assert (_code(st) == STATUS_MAXITER).all(), st
    assert (_iters(st) == 2).all()
    assert ((st & STATUS_POLISHED) == 0).all()


def test_host_ladder_strict_not_convex(runs):
    st = runs["notconvex"]["status"]
    assert (_code(st) == STATUS_NOT_CONVEX).all(), st
    assert (_iters(st) == ic.STRICT).all()


def test_host_ladder_nonfinite(runs):
    st, ref = runs["nan"]["status"], runs["tv"]
    assert _code(st)[1] == STATUS_NONFINITE
    others = np.arange(ic.BATCH) != 1
    assert (st[others] == ref["status"][others]).all()
    assert (runs["nan"]["z"][others] == ref["z"][others]).all()
