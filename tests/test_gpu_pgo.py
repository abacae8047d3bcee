"""Pose-graph optimisation on the device (rspl_pgo_*, api.PoseGraph, api.CloseLoop) against tests/pgo_ref.py, the
numpy restatement of the contract (the reference project has no loop closure).

  one linearisation (rspl_pgo_debug_system): e, b and H within 1e-12 max|ref| per array -- each entry is a sum of at
  most a few hundred O(max) products at u = 1.1e-16; delta by its backward error against the system the device
  assembled, |(H + lambda I) delta - b|_inf <= 10 n u (|H + lambda I|_inf |delta|_inf + |b|_inf);

  the LM result: the bounds of tests/pgo_cases.py (check_default), where the measured tolerances are written down."""
import numpy as np
import pytest

import pgo_cases as PC
import pgo_ref
from conftest import pkg
from rspl_slam_amd import capi

pytestmark = pytest.mark.gpu

U = 1.1e-16
NAMES = list(PC.CASES)


@pytest.fixture(scope="module")
def handle():
    return pkg.PoseGraph(max_poses=160, max_edges=1024, max_tiles=64)


@pytest.mark.parametrize("name", NAMES)
def test_system_matches_reference(handle, name):
    c = PC.case(name)
    e_ref, H_ref, b_ref, lam = PC.reference_system(name)
    e, b, H, d = pkg.pgo_system(handle, *PC.args(c), lam=lam)
    for what, got, want in (("e", e, e_ref), ("b", b, b_ref), ("H", H, H_ref)):
        err, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
        print(f"{name}: max |d {what}| = {err:.3e} of max {scale:.3e}")
        assert err <= 1e-12 * scale, (what, err, scale)
    n = len(b)
    A = H + lam * np.eye(n)
    res = float(np.abs(A @ d - b).max())
    bound = 10 * n * U * (float(np.abs(A).sum(axis=1).max()) * float(np.abs(d).max()) + float(np.abs(b).max()))
    print(f"{name}: backward error {res:.3e}, bound {bound:.3e}")
    assert np.all(np.isfinite(d)) and res <= bound, (res, bound)


@pytest.mark.parametrize("name", NAMES)
def test_solve_matches_reference(handle, name):
    c = PC.case(name)
    PC.check_default(name, handle.solve(*PC.args(c)))


def test_isolated_pose_comes_back_unchanged(handle):
    c = PC.case("isolated")
    out = handle.solve(*PC.args(c))
    np.testing.assert_array_equal(out["pose_p"][-1], c["pose_p"][-1])
    assert np.abs(out["pose_q"][-1] - c["pose_q"][-1]).max() <= 4 * U  # re-normalised by every accepted step
    np.testing.assert_array_equal(out["pose_p"][0], c["pose_p"][0])     # the fixed pose
    np.testing.assert_array_equal(out["pose_q"][0], c["pose_q"][0])
    lone = PC.lone_free_pose()  # no free pose has an edge: nothing to optimise
    out = handle.solve(*PC.args(lone))
    assert (out["status"], out["iterations"], out["trials"], out["n_free"]) == (0, 0, 0, 1)
    assert out["cost_final"] == out["cost_initial"] > 0
    np.testing.assert_array_equal(out["pose_p"], lone["pose_p"])
    np.testing.assert_array_equal(out["pose_q"], lone["pose_q"])


def test_two_solves_give_identical_bytes(handle):
    c = PC.case("n130")
    a, other, b = handle.solve(*PC.args(c)), handle.solve(*PC.args(PC.case("n33_arrow"))), handle.solve(*PC.args(c))
    for k in ("pose_q", "pose_p"):
        assert a[k].tobytes() == b[k].tobytes(), k
    for k in ("status", "iterations", "trials", "cost_initial", "cost_final", "lam"):
        assert a[k] == b[k], k


def test_ring_of_1024_poses_recovers_the_truth():
    """zero residual: the optimum is the ground truth whatever the drift; no CPU solve of this size.  1e-11:
    the 40-pose zero-residual ring comes back to 2e-14 on a CPU and this ring, closed by three loop edges, is no
    flatter per pose; the bound leaves three decades over that and sits ten below the 0.1 m of drift."""
    c = PC.big_ring(1024)
    plan = pkg.pgo_plan(c["pose_fixed"], c["edge_i"], c["edge_j"])
    assert plan["tiles_per_side"] == 64 and plan["n_filled_tiles"] < 300
    h = pkg.PoseGraph(max_poses=1024, max_edges=len(c["edge_i"]), max_tiles=plan["n_filled_tiles"])
    out = h.solve(*PC.args(c))
    dp, da = PC.pose_distance(c["truth_q"], c["truth_p"], out["pose_q"], out["pose_p"])
    print(f"1024 poses: {out['iterations']} iterations, {out['trials']} trials, F {out['cost_initial']:.3e} -> "
          f"{out['cost_final']:.3e}, dp {dp:.3e} da {da:.3e}, tiles {out['n_tiles']} -> {out['n_filled_tiles']}")
    assert out["status"] == 0  # RSPL_PGO_CONVERGED
    assert out["n_filled_tiles"] == plan["n_filled_tiles"] and out["n_free"] == 1023
    assert max(dp, da) <= 1e-11
    h.close()


def test_capacity_refusal_before_any_launch():
    h = pkg.PoseGraph(max_poses=64, max_edges=256, max_tiles=2)
    c = PC.case("n33_arrow")  # 6 filled tiles
    with pytest.raises(capi.RsplError, match=r"rc=-4"):
        h.solve(*PC.args(c))
    with pytest.raises(capi.RsplError, match=r"rc=-4"):
        h.solve(*PC.args(PC.case("n130")))  # poses
    out = h.solve(*PC.args(PC.case("n15")))  # the handle still works
    assert out["n_filled_tiles"] == 1 and out["cost_final"] < out["cost_initial"]
    h.close()


def test_close_loop_on_a_two_lap_map():
    """Two laps past the same wall (tests/pgo_cases.py: loop_scene).  Lap 2 drifts by a fixed motion per keyframe, up
    to 0.21 m; the closing keyframe's image matches lap 1's points, the vote picks the lap-1 keyframe of the same
    place, PnP gives the closing pose and the pose graph spreads the loop error over lap 2.  Every edge but the loop
    edge is measured from the current poses, so the optimum puts the closing keyframe back on lap 1 up to the share of
    the error that the loop edge itself keeps (one part in thirteen of 0.19 m, and less after the rotations settle):
    below a tenth of its error before.  Lap 1, which no loop passes through, and its points stay."""
    S = PC.loop_scene()
    M = PC.loop_map(pkg, S)
    n2 = len(S["truth"])
    last = n2 - 1
    before = PC.loop_errors(M, S)
    assert before[:n2 // 2].max() == 0 and before[last] > 0.15
    K = 128
    assert 30 <= len(S["features"]) <= K
    lm = pkg.LocalMap(max_bank_points=1024, max_local_points=1024, max_keypoints=K, max_batch=1)
    lm.store_host(np.arange(len(S["points"]), dtype=np.int32), S["descriptors"])
    F = capi.DeviceBuffer(S["features"].nbytes)
    F.upload(S["features"])
    n1 = capi.DeviceBuffer(8)
    n1.upload(np.array([len(S["features"])], np.int32))
    frame = dict(d_features=F, d_n1=n1, cam=PC.LOOP_CAM)
    pnp = pkg.PnP(max_batch=1, max_points=K)
    pg = pkg.PoseGraph(max_poses=64, max_edges=256, max_tiles=8)
    X0 = np.array([M.GetMappoint(i)[0] for i in range(0, len(S["points"]), 25)])

    ok, info = pkg.CloseLoop(M, lm, pnp, pg, frame, last, min_votes=1000)  # nobody gets a thousand votes
    assert not ok and info["stage"] == "vote" and info["candidate"] == n2 // 2 - 1 and 30 <= info["votes"] < 1000
    ok, info = pkg.CloseLoop(M, lm, pnp, pg, frame, last, min_inliers=1000)
    assert not ok and info["stage"] == "pnp" and 30 <= info["pnp_inliers"] < 1000
    np.testing.assert_array_equal(PC.loop_errors(M, S), before)  # a refused loop changes nothing

    ok, info = pkg.CloseLoop(M, lm, pnp, pg, frame, last)
    after = PC.loop_errors(M, S)
    print(f"CloseLoop: {info}\nbefore {np.round(before, 4)}\nafter  {np.round(after, 4)}")
    assert ok and info["stage"] == "done" and info["candidate"] == n2 // 2 - 1
    assert info["n_matched"] >= 0.9 * len(S["features"]) and info["pnp_inliers"] >= 0.9 * info["n_matched"]
    assert np.abs(info["pnp_twc"] - S["truth"][last][:3, 3]).max() < 1e-6  # a noise-free image
    assert info["status"] == 0 and info["cost_final"] < 0.05 * info["cost_initial"]
    assert after[last] < 0.1 * before[last]
    assert after[n2 // 2:].sum() < 0.7 * before[n2 // 2:].sum() and np.all(after[-6:] < before[-6:])
    assert after[:n2 // 2].max() < 1e-6
    X1 = np.array([M.GetMappoint(i)[0] for i in range(0, len(S["points"]), 25)])
    assert np.abs(X1 - X0).max() < 1e-6
