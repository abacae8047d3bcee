"""CPU-side checks of the F-matrix RANSAC (rspl_fm_*): the numpy restatement (tests/fm_ref.py) is pinned to the
RNG restatement already checked (oracle.pnp_subsets) and recovers ground truth on its own; the library's host
entry points -- the subsets rspl_fm_solve draws and the host instantiation of the kernel's 7-point solver
(csrc/fm_solve.hpp) -- equal it.  No GPU needed."""
import pathlib

import numpy as np
import pytest

import fm_cases as FC
import fm_ref
import oracle

ROOT = pathlib.Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def FR():
    import rspl_loader
    return rspl_loader.load().FundamentalRansac


def _match_models(got, want):
    """got's models reordered to want's (the order of a subset's models follows the null-space basis)"""
    assert len(got) == len(want)
    out, left = [], list(range(len(got)))
    for w in want:
        d = [np.abs(fm_ref.normalized(got[k]) - fm_ref.normalized(w)).max() for k in left]
        out.append(got[left.pop(int(np.argmin(d)))])
    return out


# 1 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [8, 9, 64, 300])
def test_rng_and_get_subset_equal_the_pnp_restatement(count):
    got, redraws, _ = fm_ref.subsets(count, 100, model_points=5)
    assert redraws == 0
    np.testing.assert_array_equal(got, oracle.pnp_subsets(count, 100))


# 2 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [8, 9, 64, 300, 1024])
def test_debug_subsets_equal_fm_ref(FR, count):
    p0, p1, _, _ = FC.scene(count, 0.3 if count >= 64 else 0.0, 0.0, seed=100 + count)
    want, _, _ = fm_ref.subsets(count, 1000, p0, p1)
    got = FR.debug_subsets(count, 1000, p0, p1)
    assert got.shape == (1000, 7)
    np.testing.assert_array_equal(got, want)


def test_debug_subsets_redraw_a_collinear_triple(FR):
    # 9 pairs, three of them on one line of image 0: many subsets end with a point collinear with two earlier ones
    p0, p1, _, _ = FC.scene(9, 0.0, 0.0, seed=3)
    p0 = p0.copy()
    p0[0], p0[1], p0[2] = (100.0, 100.0), (200.0, 150.0), (300.0, 200.0)
    want, redraws, _ = fm_ref.subsets(9, 1000, p0, p1)
    assert redraws > 0  # the restatement does redraw on this scene
    plain, _, _ = fm_ref.subsets(9, 1000)
    got = FR.debug_subsets(9, 1000, p0, p1)
    np.testing.assert_array_equal(got, want)
    assert not np.array_equal(want, plain)  # ... and the redraws change the sequence


def test_debug_subsets_identical_points_find_nothing(FR):
    p = np.tile([[120.0, 80.0]], (16, 1))
    want, redraws, _ = fm_ref.subsets(16, 3, p, p, max_attempts=fm_ref.MAX_ATTEMPTS)
    assert len(want) == 0 and redraws == fm_ref.MAX_ATTEMPTS
    got = FR.debug_subsets(16, 3, p, p)
    assert got.shape == (0, 7)


# 3 ------------------------------------------------------------------------------------------------------------
def _check_models(p0, p1, got, want):
    got = _match_models(got, want)
    x0 = np.concatenate([p0, np.ones((7, 1))], 1)
    x1 = np.concatenate([p1, np.ones((7, 1))], 1)
    for g, w in zip(got, want):
        assert np.abs(fm_ref.normalized(g) - fm_ref.normalized(w)).max() <= 1e-9
        G = g.reshape(3, 3)
        nF = np.linalg.norm(G)
        res = np.abs(np.einsum("ni,ij,nj->n", x1, G, x0))
        assert np.all(res <= 1e-9 * nF * np.linalg.norm(x0, axis=1) * np.linalg.norm(x1, axis=1))
        assert abs(np.linalg.det(G)) <= 1e-9 * nF ** 3


def test_debug_seven_point_equals_fm_ref(FR):
    p0, p1, _, _ = FC.scene(400, 0.3, 0.3, seed=11)
    rng = np.random.default_rng(5)
    skipped, roots = 0, {1: 0, 3: 0}
    for _ in range(200):
        idx = rng.choice(400, 7, replace=False)
        want, rel = fm_ref.seven_point(p0[idx], p1[idx])
        if rel is not None and rel <= FC.MARGIN:
            skipped += 1
            continue
        got = FR.debug_seven_point(p0[idx], p1[idx])
        assert len(got) == len(want)
        roots[len(want)] = roots.get(len(want), 0) + 1
        _check_models(p0[idx], p1[idx], got, want)
    assert skipped <= 2  # at most 1 %
    assert roots[1] > 0 and roots[3] > 0  # both branches of the cubic


@pytest.mark.parametrize("case", ["identical", "collinear", "duplicate", "huge"])
def test_debug_seven_point_degenerate_input_is_finite(FR, case):
    rng = np.random.default_rng(2)
    p0 = rng.uniform(10, 700, (7, 2))
    p1 = rng.uniform(10, 400, (7, 2))
    if case == "identical":
        p0[:] = p0[0]
        p1[:] = p1[0]
    elif case == "collinear":
        p0[:, 1] = 2 * p0[:, 0] + 1
        p1[:, 1] = 3 * p1[:, 0] - 5
    elif case == "duplicate":
        p0[3], p1[3] = p0[2], p1[2]
    else:
        p0 *= 1e30
    got = FR.debug_seven_point(p0, p1)
    assert got.shape[0] <= 3 and np.all(np.isfinite(got))


# 4 ------------------------------------------------------------------------------------------------------------
SEED = {0.0: 1, 0.3: 1, 0.6: 208}  # seeds for which fm_cases.checked_scene's precondition holds


@pytest.mark.parametrize("outliers", [0.0, 0.3, 0.6])
def test_fm_ref_recovers_the_ground_truth(outliers):
    p0, p1, inl, ref = FC.checked_scene(200, outliers, 0.0, seed=SEED[outliers])
    np.testing.assert_array_equal(ref["mask"].astype(bool), inl)
    assert ref["n_inliers"] == int(inl.sum())
    # the iteration count is what RANSACUpdateNumIters predicts from the accepted counts, in sequence
    niters, last = 1000, 0
    for it, rec in enumerate(ref["trace"]):
        assert it < niters
        if rec["accepted"] >= 0:
            best = max(c for c in rec["counts"])
            niters = fm_ref.update_num_iters(0.99, (200 - best) / 200, 7, niters)
            last = it
    # (the iteration that lowers the limit below its own index is still the last one evaluated)
    assert ref["hypotheses"] == len(ref["trace"]) == max(niters, last + 1)
    if outliers == 0.0:
        assert ref["hypotheses"] <= 5  # log(0.01) / log(1 - 1) -> 0 after the first all-inlier model


def test_fm_ref_iterations_fall_with_the_inlier_ratio():
    h = [FC.checked_scene(200, o, 0.0, seed=SEED[o])[3]["hypotheses"] for o in (0.0, 0.3, 0.6)]
    assert h[0] < h[1] < h[2]
    # the closed form at the final inlier ratio
    for o, got in zip((0.3, 0.6), h[1:]):
        want = min(1000, int(np.rint(np.log(0.01) / np.log(1 - (1 - o) ** 7))))
        assert got == want


def test_fm_ref_small_counts():
    p0, p1, _, _ = FC.scene(7, 0.0, 0.0, seed=4)
    for n in (0, 3, 6):
        r = fm_ref.find_fundamental(p0[:n], p1[:n])
        assert r["n_inliers"] == -1 and r["F"] is None and np.all(r["mask"] == 1) and len(r["mask"]) == n
    r = fm_ref.find_fundamental(p0, p1)
    assert r["n_inliers"] == 7 and r["hypotheses"] == 1 and np.all(r["mask"] == 1)


# 5 ------------------------------------------------------------------------------------------------------------
def test_header_declares_fm_api_and_keeps_the_abi_version():
    import re
    hdr = (ROOT / "include" / "rspl.h").read_text()
    assert "#define RSPL_ABI_VERSION 2" in hdr
    names = set(re.findall(r"\b(rspl_[a-z0-9_]+)\s*\(", hdr))
    from rspl_slam_amd import capi
    lib = capi.load()
    for n in ("rspl_fm_create", "rspl_fm_destroy", "rspl_fm_solve", "rspl_fm_enqueue", "rspl_fm_fetch",
              "rspl_fm_debug_subsets", "rspl_fm_debug_seven_point", "rspl_fm_debug_hypotheses"):
        assert n in names and n in capi.EXPORTS and hasattr(lib, n)
    for s in ("rspl_fm_config", "rspl_fm_problem", "rspl_fm_result", "rspl_fm_frame"):
        assert re.search(r"}\s*%s;" % s, hdr), s
    assert "is not implemented" not in hdr[hdr.index("PointMatching (src/point_matching.cc)"):hdr.index("rspl_pm_match(")]
