"""GPU FrameOptimization (rspl_frame_optimize) vs the fp64 CPU restatement (oracle/ba.c
orc_frame_opt) on the same inputs: identical round counts, inlier counts and inlier flags,
poses within 1e-9 m / rad, per-round final chi2 within rtol 1e-9.  LM iteration counts are NOT
compared: once a round has converged, g2o's stop test (rho == 0, or 10 rejected trials) is
decided by the last ulp of chi2, which the GPU's reduction tree and the host's sequential sum
round differently -- parity is judged on the optimum, as SURVEY.md section 8c states.
Every problem here is a generic synthetic.frame_problem.  The degenerate inputs (no inlier at all, points
behind the camera, a poor seed, a rank-deficient system) and the kernel's variants side by side (all four
frame_opt_kernel<LDS, NW> instantiations, 512 | 513 edges, 256 | 257 frames, the staging loop's tails,
empty and tiny frames on the global path) are in tests/test_gpu_pose_edges.py, to the same _compare."""
import numpy as np
import pytest

import oracle
from rspl_slam_amd import synthetic as SY
from rspl_slam_amd import ba_types as BT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fba():
    import rspl_loader
    pkg = rspl_loader.load()
    return pkg.FrameBA(max_batch=512, max_edges=1 << 18, max_points=1 << 18)


def _compare(r, ref, tol=1e-9):
    assert (r.rounds, r.n_inliers) == (ref.rounds, ref.n_inliers)
    assert [i > 0 for i in r.iterations] == [i > 0 for i in ref.iterations]
    np.testing.assert_allclose(r.chi2, ref.chi2, rtol=1e-9, atol=1e-9)
    assert np.abs(r.pose_p - ref.pose_p).max() < tol
    s = np.sign(np.dot(r.pose_q, ref.pose_q))
    assert np.abs(r.pose_q - s * ref.pose_q).max() < tol
    for k in ("mono", "stereo"):
        np.testing.assert_array_equal(r.inlier[k], ref.inlier[k], err_msg=k)


@pytest.mark.parametrize("seed,n,outl", [(0, 300, 0.1), (1, 400, 0.05), (2, 120, 0.2), (3, 2048, 0.1)])
def test_frame_matches_oracle(fba, seed, n, outl):
    prob, gt = SY.frame_problem(n_points=n, outlier_frac=outl, seed=seed)
    _compare(fba.run([prob])[0], oracle.frame_opt(prob))


def test_batch_of_mixed_frames(fba):
    probs = [SY.frame_problem(n_points=n, outlier_frac=o, seed=100 + i, stereo_frac=sf)[0]
             for i, (n, o, sf) in enumerate([(50, 0.1, 0.0), (300, 0.1, 1.0), (9, 0.0, 0.5), (640, 0.15, 0.6),
                                            (1, 0.0, 0.5), (64, 0.3, 0.5), (65, 0.0, 0.5), (200, 0.1, 0.6)])]
    res = fba.run(probs)
    for p, r in zip(probs, res):
        _compare(r, oracle.frame_opt(p))


def test_inlier_flags_in_and_empty(fba):
    prob, _ = SY.frame_problem(n_points=150, outlier_frac=0.1, seed=7)
    prob.mono["inlier"][::3] = 0          # Constraint::inlier false on entry: recomputed at the estimate
    prob.stereo["inlier"][1::4] = 0
    empty = BT.FrameProblem(cameras=prob.cameras, pose_q=[0, 0, 0, 1], pose_p=[0.5, 0, 0], points=np.zeros((0, 3)))
    r = fba.run([prob, empty])
    _compare(r[0], oracle.frame_opt(prob))
    _compare(r[1], oracle.frame_opt(empty))


def test_large_batch(fba):
    # C4-style throughput shape: many independent frames in one launch; a sample checked
    probs = [SY.frame_problem(n_points=400, outlier_frac=0.1, seed=1000 + i)[0] for i in range(256)]
    res = fba.run(probs)
    for i in range(0, 256, 37):
        _compare(res[i], oracle.frame_opt(probs[i]))


def test_reference_signature_in_place():
    import rspl_loader
    pkg = rspl_loader.load()
    prob, gt = SY.frame_problem(n_points=200, outlier_frac=0.1, seed=11)
    poses = {42: BT.Pose3d(False, prob.pose_p.copy(), prob.pose_q.copy())}
    points = {100 + i: BT.Position3d(True, prob.points[i]) for i in range(prob.points.shape[0])}
    cams = [BT.Camera(*prob.cameras[0])]
    mono = [BT.MonoPointConstraint(42, 100 + int(j), 0, o) for j, o in zip(prob.mono["lm"], prob.mono["obs"])]
    stereo = [BT.StereoPointConstraint(42, 100 + int(j), 0, o) for j, o in zip(prob.stereo["lm"], prob.stereo["obs"])]
    n = pkg.FrameOptimization(poses, points, cams, mono, stereo, BT.OptimizationConfig())
    ref = oracle.frame_opt(prob)
    assert n == ref.n_inliers
    assert np.abs(poses[42].p - ref.pose_p).max() < 1e-9
    assert [c.inlier for c in mono] == list(ref.inlier["mono"].astype(bool))
    assert [c.inlier for c in stereo] == list(ref.inlier["stereo"].astype(bool))


def test_frame_alone_and_in_a_large_batch(fba):
    """The wave count per frame follows the batch size (4 waves for <= 256 frames, 1 above), which
    changes the summation order of H / b / chi2: the same frame solved alone and inside a batch of
    300 agrees to the oracle tolerances (rounds, inlier flags, pose 1e-9), not bitwise."""
    probs = [SY.frame_problem(n_points=400, outlier_frac=0.1, seed=2000 + i)[0] for i in range(300)]
    alone = fba.run(probs[:1])[0]
    batch = fba.run(probs)[0]
    _compare(alone, batch)


def test_create_destroy_cycle():
    """20 handles of the smallest capacities created and destroyed (device arena, pinned arena, stream), then
    one more: its result equals the first handle's bit for bit."""
    import rspl_loader
    from helpers import assert_same, cycle_handle
    pkg = rspl_loader.load()
    prob, gt = SY.frame_problem(n_points=8, outlier_frac=0.0, seed=0)
    first, last = cycle_handle(lambda: pkg.FrameBA(max_batch=1, max_edges=8, max_points=8), lambda h: h.run([prob]))
    assert first[0].n_inliers > 0
    assert_same(first, last)
