"""GPU SolvePnPWithCV and FrameOptimization on degenerate geometry and on the kernel variants the generic tests
(tests/test_gpu_pnp.py, tests/test_gpu_frame.py) never reach, against the same fp64 CPU oracle and to the same
contracts -- their `_compare` functions are imported, not restated:
  PnP    (n_inliers, hypotheses evaluated) equal, masks equal, R within 1e-9, t within 1e-8 m; every hypothesis'
         inlier count equal (-1 = the minimal solve failed) and its pose bit-equal where the solve succeeded;
  frame  rounds, inlier counts and flags equal, the `iterations > 0` pattern equal, chi2 rtol 1e-9, pose 1e-9.
The cases are tests/pose_cases.py's; tests/test_pose_cases_cpu.py proves on the oracle that each reaches its path
(failed minimal solves and the `c < 0` skip of pnp_final_kernel, its `best < 0` return, idle waves in the last
workgroup of pnp_hyp_kernel, the [B][kMaxIters][12] hypothesis indexing at frame > 0; in frame_opt_kernel the four
<LDS, NW> instantiations, the staging loop's tails, rounds without an active edge, points behind the camera,
optimize(10) exhausted, a rank-2 system).

One check uses none of the project's C: the sum of squared reprojection errors over the returned inlier set in
np.longdouble, at the GPU's pose and at the oracle's.  The GPU's may exceed the oracle's by at most 10 x the
relative cost difference between the mirror oracle and the independent one (oracle.pnp(independent=True)) on the
same case -- the spread of two correct solvers that stop at the same optimum -- measured in the test.

One tolerance is not the contract's 1e-9: the pose of the 10- and 12-edge frames (the 10-edge frame on the global
path, the frames that fill the 256- and 257-frame batches).  The oracle alone moves such a frame's pose by up to
6e-9 when its edges are reordered, with chi2 equal to 1e-14 (pose_cases.order_spread; measured on the device: the
10-edge frame 2.6e-9 from the oracle, which is exactly the oracle's own 2.6e-9 spread on it), so these frames are
held to 10 x that oracle-only spread, floored at 1e-9: the 10-edge frame to its own, the 12-edge fill frames to
the largest over all of them.  Every named case keeps 1e-9.

Every comparison prints a ``POSE_PARITY`` line with what it measured and the tolerance it applied
(profiles/pose_edge_parity.json is collected from them)."""
import functools
import json

import numpy as np
import pytest

import oracle
import pose_cases as PC
from test_gpu_frame import _compare as frame_compare
from test_gpu_pnp import _compare as pnp_compare

pytestmark = pytest.mark.gpu

PNP_TOL = "tests/test_gpu_pnp.py::_compare: R 1e-9, t 1e-8 m"
FRAME_TOL = "tests/test_gpu_frame.py::_compare: pose 1e-9, chi2 rtol 1e-9"
SPREAD_TOL = "10 x oracle_spread (the oracle's own pose change when its edges are reordered, pose_cases.order_spread)"


@pytest.fixture(scope="module")
def pnp():
    import rspl_loader
    return rspl_loader.load().PnP(max_batch=3, max_points=512)


@pytest.fixture(scope="module")
def fba():
    import rspl_loader
    return rspl_loader.load().FrameBA(max_batch=257, max_edges=4608, max_points=4608)


PNP_CASES = PC.pnp_cases()
FRAME_CASES = PC.frame_cases()


@functools.lru_cache(maxsize=None)
def _pnp_ref(name, iterations=100):
    case = PNP_CASES[name] if name in PNP_CASES else PC.generic()
    return oracle.pnp(*case, iterations=iterations)


@functools.lru_cache(maxsize=None)
def _pnp_ref_hyp(name, iterations=100):
    case = PNP_CASES[name] if name in PNP_CASES else PC.generic()
    return oracle.pnp_hypotheses(*case, iterations)


@functools.lru_cache(maxsize=None)
def _frame_ref(name):
    return oracle.frame_opt(FRAME_CASES[name])


def _pnp_check(name, g, ref):
    """POSE_PARITY line, then tests/test_gpu_pnp.py's contract"""
    n, R, t, inl, used = g
    rec = {"case": name, "solver": "pnp", "n_inliers": [int(n), int(ref[0])], "hypotheses": [int(used), int(ref[4])],
           "rotation_diff": float(np.abs(R - ref[1]).max()) if n > 0 else None,
           "translation_diff": float(np.abs(t - ref[2]).max()) if n > 0 else None,
           "tolerance": [1e-9, 1e-8], "tolerance_source": PNP_TOL}
    print("POSE_PARITY", json.dumps(rec))
    pnp_compare(g, ref)


def _pose_diff(r, ref):
    s = np.sign(np.dot(r.pose_q, ref.pose_q))
    return float(np.abs(r.pose_p - ref.pose_p).max()), float(np.abs(r.pose_q - s * ref.pose_q).max())


@functools.lru_cache(maxsize=None)
def _fill_spread():
    """the largest oracle-only spread (pose_cases.order_spread) over the 12-edge frames that fill the large batches"""
    return max(PC.order_spread(PC.fill_frame(i)) for i in range(1, 257))


def _small_frame_tolerance(prob):
    """(pose tolerance, oracle spread) of a frame of 10 or 12 edges.  Such a frame cannot be held to 1e-9: the
    oracle ALONE moves its pose by up to 6e-9 when its edges are reordered (pose_cases.order_spread: the stop test
    is decided by the last ulp of chi2 and the frame's weakest direction is flat), with chi2 equal to 1e-14.  That
    is conditioning, not a defect, so the tolerance is 10 x that oracle-only spread, floored at the contract's
    1e-9; everything else of the contract (rounds, flags, iteration pattern, chi2 rtol 1e-9) is unchanged.
    The 12-edge fill frames are one case with one spread, the largest over all of them: eight orders sample a
    single frame's stop points, they do not list them (one fill frame whose eight orders agreed to 1e-10 came back
    from the device 5.3e-9 away, inside what its neighbours' orders show)."""
    spread = _fill_spread() if PC.n_edges(prob) == 12 else PC.order_spread(prob)
    return max(1e-9, 10 * spread), spread


def _frame_check(name, r, ref, small=None):
    """POSE_PARITY line, then tests/test_gpu_frame.py's contract (small: the problem, for a frame of 10 or 12 edges
    held to _small_frame_tolerance)"""
    c, rc = np.array(r.chi2), np.array(ref.chi2)
    dp, dq = _pose_diff(r, ref)
    rec = {"case": name, "solver": "frame", "n_inliers": [int(r.n_inliers), int(ref.n_inliers)],
           "iterations": [list(r.iterations), list(ref.iterations)], "position_diff": dp, "quaternion_diff": dq,
           "chi2_rel_diff": float((np.abs(c - rc) / np.maximum(np.abs(rc), 1.0)).max()),
           "tolerance": 1e-9, "tolerance_source": FRAME_TOL}
    if small is not None:
        rec["tolerance"], rec["oracle_spread"] = _small_frame_tolerance(small)
        if rec["tolerance"] > 1e-9:
            rec["tolerance_source"] = SPREAD_TOL
    print("POSE_PARITY", json.dumps(rec))
    frame_compare(r, ref, rec["tolerance"])


def _fill_check(name, probs, res, refs):
    """the 12-edge frames that fill a large batch, each against the oracle at _small_frame_tolerance; one
    POSE_PARITY line with the largest difference"""
    tol, spread = _small_frame_tolerance(probs[0])
    worst = 0.0
    for p, r, ref in zip(probs, res, refs):
        assert PC.n_edges(p) == 12
        worst = max(worst, *_pose_diff(r, ref))
        frame_compare(r, ref, tol)
    print("POSE_PARITY", json.dumps({
        "case": name, "solver": "frame", "frames": len(probs), "pose_diff": worst, "tolerance": tol,
        "oracle_spread": spread, "tolerance_source": SPREAD_TOL if tol > 1e-9 else FRAME_TOL}))


def _hypotheses_equal(got, ref):
    """counts equal, -1 included; poses bit-equal where the minimal solve succeeded (a failed wave leaves its
    R | t unwritten)"""
    (cg, pg), (cc, pc) = got, ref
    np.testing.assert_array_equal(cg, cc)
    ok = cc >= 0
    np.testing.assert_array_equal(pg[ok], pc[ok])


# ----------------------------------------------------------------------------------------------------------
# SolvePnPWithCV
# ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PNP_CASES))
def test_pnp_case_matches_oracle(pnp, name):
    g = pnp.solve([PNP_CASES[name]])[0]
    _pnp_check(name, g, _pnp_ref(name))
    if name.split("[")[0] in PC.HYPOTHESIS_CASES:
        _hypotheses_equal(pnp.debug_hypotheses(0), _pnp_ref_hyp(name))
    if name in ("world_plane_z0", "all_outliers"):
        assert (g[0], g[4]) == (0, 100) and not g[3].any()


def test_pnp_hypotheses_in_a_batch(pnp):
    """the hypothesis arrays of the frames behind frame 0: [B][kMaxIters][12] poses, [B][kMaxIters] counts"""
    tilted = f"tilted_plane[{PC.TILTED_PLANE_SEEDS[2]}]"  # a seed with failed hypotheses
    assert (_pnp_ref_hyp(tilted)[0] < 0).any()
    frames = [PC.generic(), PNP_CASES[tilted], PC.seven_points()]
    res = pnp.solve(frames)
    _pnp_check("batch/generic", res[0], _pnp_ref("generic"))
    _pnp_check("batch/" + tilted, res[1], _pnp_ref(tilted))
    _hypotheses_equal(pnp.debug_hypotheses(0), _pnp_ref_hyp("generic"))
    _hypotheses_equal(pnp.debug_hypotheses(1), _pnp_ref_hyp(tilted))
    assert not np.array_equal(_pnp_ref_hyp("generic")[1], _pnp_ref_hyp(tilted)[1])  # frame 0's would not pass for frame 1's
    counts, poses = pnp.debug_hypotheses(2)  # 7 correspondences: no hypothesis was drawn
    assert len(counts) == 0 and poses.shape == (0, 12)
    assert res[2][0] == 0 and res[2][4] == 0 and not res[2][3].any()


@pytest.mark.parametrize("iterations", [1, 5, 101, 128])
def test_pnp_iteration_counts(pnp, iterations):
    """1 and kMaxIters = 128 are the ends of the accepted range; 1, 5 and 101 leave waves of the last
    pnp_hyp_kernel workgroup (kHypWaves = 4) idle"""
    g = pnp.solve([PC.generic()], iterations=iterations)[0]
    _pnp_check(f"iterations[{iterations}]", g, _pnp_ref("generic", iterations))
    cg, pg = pnp.debug_hypotheses(0)
    assert len(cg) == iterations
    if iterations == 101:
        _hypotheses_equal((cg, pg), _pnp_ref_hyp("generic", 101))


def test_pnp_refuses_129_iterations(pnp):
    import rspl_loader
    with pytest.raises(rspl_loader.load().capi.RsplError, match=r"rc=-1\)") as e:  # RSPL_E_ARG
        pnp.solve([PC.generic()], iterations=129)
    assert "iterations must be 1..128" in str(e.value)
    _pnp_check("after the refusal", pnp.solve([PC.generic()])[0], _pnp_ref("generic"))  # the handle is intact


@pytest.mark.parametrize("name", [f"tilted_plane[{PC.TILTED_PLANE_SEEDS[0]}]", "c5_camera", "generic"])
def test_pnp_objective_in_numpy(pnp, name):
    case = PNP_CASES[name] if name in PNP_CASES else PC.generic()
    n, R, t, inl, _ = pnp.solve([case])[0]
    mirror, indep = _pnp_ref(name), oracle.pnp(*case, independent=True)
    np.testing.assert_array_equal(inl, mirror[3])
    np.testing.assert_array_equal(indep[3], mirror[3])
    assert n > 0
    c_gpu = PC.reprojection_cost(*case, R, t, inl)
    c_mirror = PC.reprojection_cost(*case, mirror[1], mirror[2], inl)
    c_indep = PC.reprojection_cost(*case, indep[1], indep[2], inl)
    spread = abs(c_mirror - c_indep) / c_mirror
    margin = 10 * spread
    excess = (c_gpu - c_mirror) / c_mirror
    print("POSE_PARITY", json.dumps({
        "case": "objective/" + name, "solver": "pnp", "cost_gpu": float(c_gpu), "cost_oracle": float(c_mirror),
        "relative_excess": float(excess), "oracle_spread": float(spread), "tolerance": float(margin),
        "tolerance_source": "10 x the relative cost difference of the mirror and the independent oracle (oracle_spread)"}))
    assert excess <= margin, (float(excess), float(margin))


# ----------------------------------------------------------------------------------------------------------
# FrameOptimization
# ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FRAME_CASES))
def test_frame_case_matches_oracle(fba, name):
    r = fba.run([FRAME_CASES[name]])[0]
    ref = _frame_ref(name)
    _frame_check(name, r, ref)
    assert tuple(i > 0 for i in r.iterations) == tuple(i > 0 for i in ref.iterations)
    if name == "all_outliers":
        assert tuple(r.iterations[1:]) == (0, 0, 0) and tuple(r.chi2[1:]) == (0.0, 0.0, 0.0) and r.n_inliers == 0
    if name == "behind_camera":
        assert (PC.z_camera(FRAME_CASES[name], r) < 0).sum() >= 10


def test_frame_four_kernel_instantiations(fba):
    """frame_kernels.hip::optimize: NW = 1 above 256 frames, else 4; LDS while the batch's largest frame has at most
    kLdsEdges = 512 edges.  A: frame_opt_kernel<true,4>, B: <false,4>, C: <true,1>, D: <false,1>
    (pose_cases.variant_batches; test_pose_cases_cpu.py asserts the four selections)."""
    batches = PC.variant_batches()
    assert {k: v[0] for k, v in batches.items()} == {"A": "<true,4>", "B": "<false,4>", "C": "<true,1>", "D": "<false,1>"}
    refs = {}

    def ref(p):  # one oracle run per distinct problem (C and D share 256 of them)
        if id(p) not in refs:
            refs[id(p)] = oracle.frame_opt(p)
        return refs[id(p)]

    res = {}
    for name, (variant, probs) in batches.items():
        res[name] = fba.run(probs)
        assert len(res[name]) == len(probs)
        # frame 0, the staging_tails frames and the 513-edge frame: the contract as it stands
        fill = [i for i, p in enumerate(probs) if PC.n_edges(p) == 12]
        for i, (p, r) in enumerate(zip(probs, res[name])):
            if i not in fill:
                _frame_check(f"variant {name} {variant} frame {i} ({PC.n_edges(p)} edges)", r, ref(p))
        if fill:  # and every 12-edge frame between them
            _fill_check(f"variant {name} {variant} 12-edge frames", [probs[i] for i in fill],
                        [res[name][i] for i in fill], [ref(probs[i]) for i in fill])
    frame_compare(res["C"][0], res["D"][0])  # the same 400-edge frame through <true,1> and <false,1>
    frame_compare(res["B"][0], res["D"][-1])  # the same 513-edge frame through <false,4> and <false,1>


def test_frame_batch_256_against_257(fba):
    """four waves per frame up to 256 frames, one wave above: the same first frame either side of the switch"""
    first = FRAME_CASES["behind_camera"]
    fill = [PC.fill_frame(i) for i in range(1, 257)]
    ref = _frame_ref("behind_camera")
    r256 = fba.run([first] + fill[:255])
    r257 = fba.run([first] + fill)
    assert len(r256) == 256 and len(r257) == 257
    _frame_check("batch of 256 <true,4> frame 0", r256[0], ref)
    _frame_check("batch of 257 <true,1> frame 0", r257[0], ref)
    frame_compare(r256[0], r257[0])
    sample = [0, 127, 254]  # 12-edge frames behind it, either side of the switch, and the 257th frame
    refs = [oracle.frame_opt(fill[i]) for i in sample + [255]]
    _fill_check("batch of 256 <true,4> 12-edge frames", [fill[i] for i in sample], [r256[i + 1] for i in sample], refs[:3])
    _fill_check("batch of 257 <true,1> 12-edge frames", [fill[i] for i in sample + [255]],
                [r257[i + 1] for i in sample + [255]], refs)


def test_frame_empty_and_tiny_frames_on_global_path(fba):
    """a 513-edge frame puts the whole batch on the global-memory path: the frames behind it take their errors,
    levels and flags from a.err + 4 * e0, a.level + e0, a.inl + e0 with e0 = 513, 513, 514, 523"""
    probs = [PC.edges(513), PC.empty_frame(), PC.tiny_frame(1), PC.tiny_frame(9), PC.tiny_frame(10)]
    assert [PC.n_edges(p) for p in probs] == [513, 0, 1, 9, 10]
    res = fba.run(probs)
    refs = [oracle.frame_opt(p) for p in probs]
    for p, r, ref in zip(probs, res, refs):
        _frame_check(f"global path, {PC.n_edges(p)} edges", r, ref, small=p if PC.n_edges(p) == 10 else None)
    assert [r.rounds for r in res] == [4, 1, 1, 1, 4]  # fewer than 10 edges: one round
    assert res[1].n_inliers == 0 and res[1].iterations[0] == 0
    np.testing.assert_allclose(res[1].pose_p, probs[1].pose_p, atol=1e-15)
