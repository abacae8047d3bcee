"""The pose solvers' edge cases (tests/pose_cases.py) on the CPU oracle alone: every case reaches the path it is
meant to reach -- failed minimal solves, an empty consensus, LM rounds without an active edge, exhausted
optimize(10) calls, points behind the camera, the 512 | 513 edge counts -- with the committed seeds.  The device
tests (tests/test_gpu_pose_edges.py) compare the kernels with the same oracle on the same cases; these assertions
keep a later change to a generator from quietly turning one of them into a generic problem."""
import numpy as np
import pytest

import oracle
import pose_cases as PC


def _failed(case):
    counts, _ = oracle.pnp_hypotheses(*case, 100)
    return int((counts < 0).sum())


def test_tilted_plane_has_failed_hypotheses():
    failed = []
    for s in PC.TILTED_PLANE_SEEDS:
        case = PC.tilted_plane(s)
        n, R, t, inl, used = oracle.pnp(*case)
        assert n > 0 and inl.sum() == n and np.isfinite(R).all() and np.isfinite(t).all(), s
        failed.append(_failed(case))
    assert max(failed) >= 1, failed  # the `c < 0` skip of the acceptance loop runs beside accepted hypotheses
    # the points are coplanar in the world (rank 2 after centring, to float rounding)
    X = PC.tilted_plane(PC.TILTED_PLANE_SEEDS[0])[1]
    sv = np.linalg.svd(X - X.mean(0), compute_uv=False)
    assert sv[2] < 1e-6 * sv[1]


@pytest.mark.parametrize("seed", PC.REPEATED_POINT_SEEDS)
def test_repeated_point_fails_most_hypotheses(seed):
    case = PC.repeated_point(seed)
    K, X, kp = case
    assert (X[:40] == X[0]).all() and (kp[:40] == kp[0]).all() and len(X) == 60
    assert _failed(case) >= 40
    a, b = oracle.pnp(*case), oracle.pnp(*case, independent=True)
    assert a[0] > 0
    # only seeds on which the two eigen solvers choose the same consensus: the GPU follows the mirror, and a
    # case decided inside EPnP's degenerate null space would pin an order of operations, not a result
    assert a[0] == b[0]
    np.testing.assert_array_equal(a[3], b[3])


def test_world_plane_z0_fails_every_hypothesis():
    case = PC.world_plane_z0()
    assert (case[1][:, 2] == 0.0).all() and len(case[1]) == 120
    counts, _ = oracle.pnp_hypotheses(*case, 100)
    assert (counts == -1).all() and len(counts) == 100
    n, R, t, inl, used = oracle.pnp(*case)
    assert (n, used) == (0, 100) and not inl.any()


def test_pnp_all_outliers_has_no_consensus():
    case = PC.pnp_all_outliers()
    counts, _ = oracle.pnp_hypotheses(*case, 100)
    n, R, t, inl, used = oracle.pnp(*case)
    assert n == 0 and used == 100 and not inl.any()
    assert counts.max() <= 4  # never above RANSAC's floor of 4: `best < 0` at the end


@pytest.mark.parametrize("n", PC.COUNT_EDGES)
def test_count_edges_solve(n):
    K, X, kp = PC.count_edge(n)
    assert len(X) == len(kp) == n
    assert oracle.pnp(K, X, kp)[0] > 0  # a real solve (inlier count, refinement), not an empty consensus


def test_c5_camera_is_the_scaled_euroc_camera():
    K, X, kp = PC.c5_camera()
    assert len(X) == 300 and kp[:, 0].max() > 752 and kp[:, 1].max() > 480  # the wide image is used
    np.testing.assert_allclose(K[0] / K[2], 435.2046959714599 / 367.4517211914062)
    assert oracle.pnp(K, X, kp)[0] > 200


def test_pnp_inputs_are_float_rounded():
    for name, (K, X, kp) in PC.pnp_cases().items():
        assert (X == X.astype(np.float32)).all() and (kp == kp.astype(np.float32)).all(), name


def test_frame_all_outliers_rounds_without_active_edges():
    prob = PC.frame_all_outliers()
    assert PC.n_edges(prob) == 150
    r = oracle.frame_opt(prob)
    assert r.iterations[0] > 0 and tuple(r.iterations[1:]) == (0, 0, 0)
    assert r.n_inliers == 0 and r.rounds == 4
    assert tuple(r.chi2[1:]) == (0.0, 0.0, 0.0)


def test_poor_seed_exhausts_optimize():
    r = oracle.frame_opt(PC.poor_seed())
    assert sum(i == 10 for i in r.iterations) >= 2, r.iterations
    assert r.n_inliers > 100


def test_one_point_mono_is_rank_deficient():
    prob = PC.one_point_mono()
    assert prob.n_edges("mono") == 12 and prob.n_edges("stereo") == 0 and len(prob.points) == 1
    r = oracle.frame_opt(prob)
    assert 0 in r.iterations, r.iterations
    assert np.isfinite(r.pose_p).all() and np.isfinite(r.pose_q).all()


def test_behind_camera_points_stay_behind():
    prob = PC.behind_camera()
    r = oracle.frame_opt(prob)
    z = PC.z_camera(prob, r)
    assert (z < 0).sum() >= 10 and (z != 0).all()
    assert np.isfinite(r.pose_p).all() and np.isfinite(r.pose_q).all() and r.rounds == 4 and r.n_inliers > 100


def test_edge_counts_straddle_the_lds_capacity():
    assert PC.n_edges(PC.edges(512)) == 512 and PC.n_edges(PC.edges(513)) == 513
    # the same seed: the first 512 points and observations are the same
    a, b = PC.edges(512), PC.edges(513)
    np.testing.assert_array_equal(a.points, b.points[:512])
    assert [PC.n_edges(PC.staging_tail(n)) for n in PC.STAGING_TAILS] == list(PC.STAGING_TAILS)


def test_small_frames_are_ill_conditioned_by_the_oracles_own_measure():
    """Why the device tests hold 10- and 12-edge frames to 10 x order_spread and not to 1e-9: the oracle, given the
    same 10-edge frame with its edges reordered, returns a pose more than 1e-9 away at the same chi2, and so do
    12-edge frames -- while a 150-edge frame moves by 1e-13."""
    import oracle as O
    p = PC.tiny_frame(10)
    assert PC.order_spread(p) > 1e-9
    chi = [O.frame_opt(PC.reordered(p, k)).chi2[3] for k in range(8)] + [O.frame_opt(p).chi2[3]]
    assert (max(chi) - min(chi)) / max(chi) < 1e-12
    fill = [PC.order_spread(PC.fill_frame(i)) for i in range(1, 41)]
    assert max(fill) > 1e-9 and max(fill) < 1e-7, max(fill)
    assert PC.order_spread(PC.behind_camera()) < 1e-11 and PC.order_spread(PC.poor_seed()) < 1e-11


def test_variant_batches_select_four_kernels():
    """frame_kernels.hip::optimize chooses by (batch > 256, largest frame > kLdsEdges = 512)"""
    got = {}
    for name, (variant, probs) in PC.variant_batches().items():
        lds = max(PC.n_edges(p) for p in probs) <= 512
        waves = 1 if len(probs) > 256 else 4
        got[name] = f"<{'true' if lds else 'false'},{waves}>"
        assert got[name] == variant, name
    assert sorted(got.values()) == ["<false,1>", "<false,4>", "<true,1>", "<true,4>"]
    b = PC.variant_batches()
    assert len(b["C"][1]) == len(b["D"][1]) == 257
    assert [PC.n_edges(p) for p in b["C"][1][:5]] == [400, 74, 75, 85, 86]
    assert PC.n_edges(b["D"][1][-1]) == 513 and PC.n_edges(b["C"][1][-1]) == 12
