"""CPU-side checks of loop closure (rspl_pgo_*, rspl_map_pose_graph / _apply_pose_graph / _loop_candidates): the
boundary is declared and bound; the restatement tests/pgo_ref.py has exact Jacobians (central differences) and finds
the optimum an independent optimiser finds (scipy.optimize.least_squares); the tile plan's counts; the host twin
rspl_pgo_debug_host against pgo_ref within the bounds of tests/pgo_cases.py; every refusal and every allowed edge
case of the contract; the three map calls against plain-Python restatements; tests/c/pgo_check.cpp from C++.
No GPU needed.

Parity is with this project's restatement: the reference has no loop closure."""
import pathlib
import re
import subprocess

import numpy as np
import pytest

import pgo_cases as PC
import pgo_ref

ROOT = pathlib.Path(__file__).resolve().parents[1]
FUNCS = ("rspl_pgo_create", "rspl_pgo_destroy", "rspl_pgo_solve", "rspl_pgo_debug_host", "rspl_pgo_debug_plan",
         "rspl_pgo_debug_system", "rspl_map_pose_graph", "rspl_map_apply_pose_graph", "rspl_map_loop_candidates")
STRUCTS = {"rspl_pgo_config": "PgoConfig", "rspl_pgo_problem": "PgoProblem", "rspl_pgo_params": "PgoParams",
           "rspl_pgo_result": "PgoResult"}


@pytest.fixture(scope="module")
def pkg():
    import rspl_loader
    return rspl_loader.load()


# 1: the boundary -----------------------------------------------------------------------------------------------
def test_header_declares_pgo_api_and_keeps_abi_2():
    hdr = (ROOT / "include" / "rspl.h").read_text()
    names = set(re.findall(r"\b(rspl_[a-z0-9_]+)\s*\(", hdr))
    for n in FUNCS:
        assert n in names
    for s in STRUCTS:
        assert re.search(r"}\s*%s;" % s, hdr), s
    assert "#define RSPL_ABI_VERSION 2" in hdr


def test_capi_binds_pgo_api(pkg):
    lib = pkg.capi.load()
    for n in FUNCS:
        assert n in pkg.capi.EXPORTS and hasattr(lib, n)
    for n in ("PoseGraph", "pgo_host", "pgo_plan", "pgo_system", "CloseLoop"):
        assert callable(getattr(pkg, n))
    for n in ("PoseGraph", "ApplyPoseGraph", "LoopCandidates"):
        assert callable(getattr(pkg.mapping.Map, n))


def test_pgo_check_program_and_struct_layouts(pkg):
    """tests/c/pgo_check.cpp: the host twin, the plan, the refusals and the map calls from C++ (tests/c/pgo_check.mk;
    `pgo_check_san` there is the same program under ASan + UBSan); its sizeof / offsetof lines against ctypes"""
    subprocess.run(["make", "-C", str(ROOT / "tests" / "c"), "-f", "pgo_check.mk", "pgo_check"], check=True,
                   capture_output=True)
    r = subprocess.run([str(ROOT / "tests" / "c" / "build" / "pgo_check")], capture_output=True, text=True)
    assert r.returncode == 0 and "pgo_check: ok" in r.stdout, r.stdout + r.stderr
    sizes = dict(re.findall(r"^sizeof (\w+) (\d+)$", r.stdout, re.M))
    offsets = {(s, f): int(o) for s, f, o in re.findall(r"^offsetof (\w+)\.(\w+) (\d+)$", r.stdout, re.M)}
    n_fields = 0
    for cname, pyname in STRUCTS.items():
        S = getattr(pkg.capi, pyname)
        assert int(sizes[cname]) == __import__("ctypes").sizeof(S), cname
        for f, _ in S._fields_:
            assert offsets[(cname, f.rstrip("_"))] == getattr(S, f).offset, (cname, f)
            n_fields += 1
    assert n_fields == len(offsets) == 4 + 10 + 2 + 11


# 2: the restatement --------------------------------------------------------------------------------------------
def test_reference_jacobians_against_central_differences():
    """residual angles of 2.0 to 2.6 rad, h = 1e-6: rounding u |e| / h is about 3e-10 per entry, truncation h^2 about
    1e-12; the bound is 5e-9"""
    rng = np.random.default_rng(5)
    worst, h = 0.0, 1e-6
    for angle in (2.0, 2.3, 2.6, 1e-7, 0.3):
        qi, qj = (pgo_ref.qexp(rng.standard_normal(3)) for _ in range(2))
        pi, pj = rng.standard_normal(3), rng.standard_normal(3)
        axis = rng.standard_normal(3)
        qz = pgo_ref.qmul(pgo_ref.qmul(pgo_ref.qconj(qi), qj), pgo_ref.qexp(angle * axis / np.linalg.norm(axis)))
        pz = rng.standard_normal(3)
        e, Ji, Jj = pgo_ref.edge_jacobians(qi, pi, qj, pj, qz, pz)
        if angle >= 2.0:
            assert abs(np.linalg.norm(e[3:]) - angle) < 1e-9
        for J, side in ((Ji, 0), (Jj, 1)):
            for k in range(6):
                d = np.zeros(6)
                d[k] = h
                out = []
                for s in (1, -1):
                    a = pgo_ref.pose_update(qi, pi, s * d) if side == 0 else (qi, pi)
                    b = pgo_ref.pose_update(qj, pj, s * d) if side == 1 else (qj, pj)
                    out.append(pgo_ref.edge_residual(a[0], a[1], b[0], b[1], qz, pz))
                worst = max(worst, float(np.abs((out[0] - out[1]) / (2 * h) - J[:, k]).max()))
    print(f"max |J - central difference| = {worst:.3e}")
    assert worst < 5e-9


def _least_squares_cost(P, q0, p0):
    """the optimum by scipy.optimize.least_squares over increments of (q0, p0), Jacobian by central differences of
    the residuals of each pose's own edges"""
    import scipy.optimize
    fi = P.free_index()
    free = np.flatnonzero(fi >= 0)
    sw = np.sqrt(np.repeat(P.edge_w, 3, axis=1))
    touching = [np.flatnonzero((P.edge_i == i) | (P.edge_j == i)) for i in free]

    def poses(x):
        q, p = q0.copy(), p0.copy()
        for a, i in enumerate(free):
            q[i], p[i] = pgo_ref.pose_update(q0[i], p0[i], x[6 * a:6 * a + 6])
        return q, p

    def edge_res(q, p, k):
        i, j = P.edge_i[k], P.edge_j[k]
        return sw[k] * pgo_ref.edge_residual(q[i], p[i], q[j], p[j], P.edge_q[k], P.edge_p[k])

    def fun(x):
        q, p = poses(x)
        return np.concatenate([edge_res(q, p, k) for k in range(P.n_edges)])

    def jac(x):
        J, h = np.zeros((6 * P.n_edges, len(x))), 1e-6
        q, p = poses(x)
        for a, i in enumerate(free):
            for c in range(6):
                col = 6 * a + c
                out = []
                for s in (1, -1):
                    d = x[6 * a:6 * a + 6].copy()
                    d[c] += s * h
                    qs, ps = q.copy(), p.copy()
                    qs[i], ps[i] = pgo_ref.pose_update(q0[i], p0[i], d)
                    out.append([edge_res(qs, ps, k) for k in touching[a]])
                for n, k in enumerate(touching[a]):
                    J[6 * k:6 * k + 6, col] = (out[0][n] - out[1][n]) / (2 * h)
        return J

    r = scipy.optimize.least_squares(fun, np.zeros(6 * len(free)), jac=jac, method="trf", xtol=1e-14, ftol=1e-14,
                                     gtol=1e-12, max_nfev=100)
    return 2.0 * r.cost


@pytest.mark.parametrize("name", PC.NOISY)
def test_reference_finds_least_squares_cost(name):
    """equal cost: 1e-8 relative -- the Jacobian there is a central difference (1e-9 relative), and an error of the
    stationary point enters the cost squared.  The 130-pose case starts a millimetre off pgo_ref's result, the others
    from the case's initial poses, the 170 degree one from pgo_ref's result turned by 0.1 rad (a chart over increments
    of the initial poses has a singularity on its way)."""
    P, R = PC.problem(name), PC.reference(name)
    rng = np.random.default_rng(1)
    if name in ("n130", "rot170"):
        s = (1e-3, 1e-3) if name == "n130" else (0.05, 0.1)
        q0, p0 = R.pose_q.copy(), R.pose_p + s[0] * rng.standard_normal(R.pose_p.shape)
        for i in range(len(q0)):
            q0[i] = pgo_ref.qmul(q0[i], pgo_ref.qexp(s[1] * rng.standard_normal(3) / np.sqrt(3)))
        fixed = P.pose_fixed != 0
        q0[fixed], p0[fixed] = P.pose_q[fixed], P.pose_p[fixed]
    else:
        q0, p0 = P.pose_q, P.pose_p
    F = _least_squares_cost(P, q0, p0)
    print(f"{name}: least_squares {F:.16e}, pgo_ref {R.cost_final:.16e}")
    assert abs(F - R.cost_final) <= 1e-8 * R.cost_final + 1e-24


def test_reference_sparse_path_agrees_with_dense():
    for name in ("n17", "n130"):
        P, R = PC.problem(name), PC.reference(name)
        S = pgo_ref.solve(P, sparse=True)
        assert abs(S.cost_final - R.cost_final) <= 1e-10 * R.cost_final
        e, H, b = pgo_ref.linearise(P)
        es, Hs, bs = pgo_ref.linearise(P, sparse=True)
        assert np.abs(Hs.toarray() - H).max() <= 1e-12 * np.abs(H).max() and np.array_equal(b, bs)


# 3: the plan ---------------------------------------------------------------------------------------------------
def _chain(n_poses, span):
    ei = [i for i in range(n_poses) for k in range(1, span + 1) if i + k < n_poses]
    ej = [i + k for i in range(n_poses) for k in range(1, span + 1) if i + k < n_poses]
    fx = np.zeros(n_poses, np.uint8)
    fx[0] = 1
    return fx, ei, ej


def test_plan_tile_counts(pkg):
    fx, ei, ej = _chain(41, 1)                       # 40 free poses, span 1: a tile band
    pl = pkg.pgo_plan(fx, ei, ej, tile_map=True)
    assert (pl["n_free"], pl["tiles_per_side"], pl["n_tiles"], pl["n_filled_tiles"]) == (40, 3, 5, 5)
    np.testing.assert_array_equal(pl["tile_map"], [[0, -1, -1], [1, 2, -1], [-1, 3, 4]])  # column-major storage
    fx, ei, ej = _chain(81, 1)                       # 80 free, five tiles; the last pose to free pose 1: an arrow
    pl = pkg.pgo_plan(fx, ei + [80], ej + [2], tile_map=True)
    assert (pl["tiles_per_side"], pl["n_tiles"], pl["n_filled_tiles"]) == (5, 10, 12)
    assert (pl["tile_map"][4] >= 0).all() and pl["tile_map"][3, 0] == -1  # the arrow row fills, nothing else does
    fx = np.zeros(41, np.uint8)
    fx[0] = 1
    pairs = [(i, j) for i in range(41) for j in range(i + 1, 41)]  # complete
    pl = pkg.pgo_plan(fx, [a for a, _ in pairs], [b for _, b in pairs])
    assert (pl["tiles_per_side"], pl["n_tiles"], pl["n_filled_tiles"]) == (3, 6, 6)
    fx, ei, ej = _chain(4096, 8)                     # the 4096-pose chain of span 8: 511 tiles (38 MB)
    pl = pkg.pgo_plan(fx, ei, ej)
    assert (pl["n_free"], pl["tiles_per_side"], pl["n_tiles"], pl["n_filled_tiles"]) == (4095, 256, 511, 511)
    c = PC.big_ring(1024)                            # span 4 and three loop edges: a tenth of the 2080 tiles
    pl = pkg.pgo_plan(c["pose_fixed"], c["edge_i"], c["edge_j"])
    assert pl["tiles_per_side"] == 64 and pl["n_tiles"] == 64 + 63 + 1 and 128 < pl["n_filled_tiles"] < 300
    pl = pkg.pgo_plan(np.ones(3, np.uint8), [0, 1], [1, 2])  # nothing free
    assert (pl["n_free"], pl["tiles_per_side"], pl["n_filled_tiles"]) == (0, 0, 0)


# 4: the host twin ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PC.CASES))
def test_host_twin_matches_reference(pkg, name):
    c = PC.case(name)
    PC.check_default(name, pkg.pgo_host(*PC.args(c)))


def test_zero_residual_cases_recover_the_truth(pkg):
    for name in PC.ZERO:
        c = PC.case(name)
        out = pkg.pgo_host(*PC.args(c))
        dp, da = PC.pose_distance(c["truth_q"], c["truth_p"], out["pose_q"], out["pose_p"])
        assert out["status"] == 0 and out["cost_final"] < 1e-24 and max(dp, da) < 1e-12, (name, dp, da)


def _args(c, **over):
    d = dict(c, **over)
    return tuple(d[k] for k in PC.PROBLEM_KEYS)


def test_refusals(pkg):
    c = PC.case("n15")
    RsplError = pkg.capi.RsplError
    with pytest.raises(RsplError, match=r"rc=-1.*no fixed pose"):
        pkg.pgo_host(*_args(c, pose_fixed=np.zeros(16, np.uint8)))
    ej = c["edge_j"].copy()
    ej[4] = c["edge_i"][4]
    with pytest.raises(RsplError, match=r"rc=-1.*itself"):
        pkg.pgo_host(*_args(c, edge_j=ej))
    for bad in (16, -1):
        ej = c["edge_j"].copy()
        ej[4] = bad
        with pytest.raises(RsplError, match=r"rc=-1.*out of range"):
            pkg.pgo_host(*_args(c, edge_j=ej))
    # a second ring with no fixed pose of its own: a gauge freedom
    two = PC.case("two_components")
    fx = two["pose_fixed"].copy()
    fx[13] = 0
    with pytest.raises(RsplError, match=r"rc=-1.*gauge"):
        pkg.pgo_host(*_args(two, pose_fixed=fx))
    with pytest.raises(RsplError, match=r"rc=-1"):
        pkg.pgo_plan(fx, two["edge_i"], two["edge_j"])


def test_allowed_edge_cases(pkg):
    c = PC.case("isolated")
    out = pkg.pgo_host(*PC.args(c))  # a free pose without an edge comes back unchanged
    np.testing.assert_array_equal(out["pose_p"][-1], c["pose_p"][-1])
    assert np.abs(out["pose_q"][-1] - c["pose_q"][-1]).max() <= 4.4e-16
    c = PC.case("n15")
    base = pkg.pgo_host(*PC.args(c))
    # an edge between two fixed poses only adds its own cost
    fx = c["pose_fixed"].copy()
    fx[15] = 1
    ff = dict(c, pose_fixed=fx)
    a = pkg.pgo_host(*PC.args(ff))
    extra = dict(ff, edge_i=np.append(c["edge_i"], 0).astype(np.int32), edge_j=np.append(c["edge_j"], 15).astype(np.int32),
                 edge_q=np.vstack([c["edge_q"], [0, 0, 0, 1]]), edge_p=np.vstack([c["edge_p"], [0, 0, 0]]),
                 edge_w=np.vstack([c["edge_w"], [2.0, 3.0]]))
    b = pkg.pgo_host(*PC.args(extra))
    P = pgo_ref.Problem(*PC.args(extra))
    own = pgo_ref.cost_of(P, pgo_ref.residuals(P))
    Pb = pgo_ref.Problem(*PC.args(ff))
    own -= pgo_ref.cost_of(Pb, pgo_ref.residuals(Pb))
    assert own > 1 and abs(b["cost_final"] - a["cost_final"] - own) <= 1e-10 * own
    assert PC.pose_distance(a["pose_q"], a["pose_p"], b["pose_q"], b["pose_p"]) < (1e-6, 1e-6)
    # duplicate edges sum: every edge twice is every weight doubled
    twice = dict(c, **{k: np.concatenate([c[k], c[k]]) for k in PC.PROBLEM_KEYS if k.startswith("edge")})
    d = pkg.pgo_host(*PC.args(twice))
    w2 = pkg.pgo_host(*PC.args(dict(c, edge_w=2 * c["edge_w"])))
    assert abs(d["cost_final"] - 2 * base["cost_final"]) <= 1e-10 * d["cost_final"]
    assert abs(d["cost_initial"] - w2["cost_initial"]) <= 1e-12 * d["cost_initial"]
    # all poses fixed: zero iterations, converged
    z = pkg.pgo_host(*PC.args(dict(c, pose_fixed=np.ones(16, np.uint8))))
    assert (z["status"], z["iterations"], z["trials"], z["n_free"]) == (0, 0, 0, 0)
    assert z["cost_final"] == z["cost_initial"] == base["cost_initial"]
    np.testing.assert_array_equal(z["pose_p"], c["pose_p"])
    # no free pose has an edge: nothing to optimise, for the restatement too
    lone = PC.lone_free_pose()
    z = pkg.pgo_host(*PC.args(lone))
    R = pgo_ref.solve(pgo_ref.Problem(*PC.args(lone)))
    assert (z["status"], z["iterations"], z["trials"], z["n_free"]) == (0, 0, 0, 1) == (R.status, R.iterations, R.trials, 1)
    assert z["cost_final"] == z["cost_initial"] > 0 and abs(z["cost_final"] - R.cost_final) <= 1e-12 * R.cost_final
    np.testing.assert_array_equal(z["pose_p"], lone["pose_p"])
    np.testing.assert_array_equal(z["pose_q"], lone["pose_q"])
    one = pkg.pgo_host(*PC.args(c), max_iterations=1)
    assert (one["status"], one["iterations"]) == (1, 1)  # RSPL_PGO_MAX_ITERATIONS


# 5: the map calls ----------------------------------------------------------------------------------------------
def _T(yaw, t):
    T = np.eye(4)
    T[:3, :3] = pgo_ref.qmat(pgo_ref.qexp(np.array([0.0, 0.0, yaw])))
    T[:3, 3] = t
    return T


@pytest.fixture()
def small_map(pkg):
    """five keyframes (ids 0, 3, 5, 8, 20) in a chain of parents, ten points seen by overlapping frames, a line"""
    M = pkg.mapping.Map([400.0, 400.0, 320.0, 240.0, 40.0])
    ids = [0, 3, 5, 8, 20]
    poses = {f: _T(0.2 * k, [1.0 * k, 0.3 * k * k, 0.1 * k]) for k, f in enumerate(ids)}
    kps = np.tile([[10.0, 10.0, -1.0]], (12, 1))
    for k, f in enumerate(ids):
        M.InsertKeyframe(f, 0.1 * k, poses[f], kps, lines_left=[[0.0, 0.0, 10.0, 10.0]] if f == 20 else None,
                         parent_id=ids[k - 1] if k else -1)
    sees = {0: range(0, 6), 3: range(2, 8), 5: range(4, 10), 8: range(6, 10), 20: range(0, 4)}
    rng = np.random.default_rng(3)
    X = rng.uniform(-2, 2, (10, 3)) + [0, 0, 6]
    M.InsertMappoints(np.arange(100, 110), X)
    M.InsertMappoint(110, [9.0, 9.0, 9.0], pkg.mapping.BAD)
    for f, pts in sees.items():
        M.AddPointObservations(f, [100 + j for j in pts], list(range(len(pts))))
    for f in ids:
        M.UpdateFrameConnection(f)
    return M, ids, poses, sees, X


def _conn(M, f):
    return {i: w for w, i in M.GetOrderedConnections(f)}


def test_map_pose_graph_against_restatement(pkg, small_map):
    M, ids, poses, sees, X = small_map
    for min_weight in (1, 3, 1000):
        G = M.PoseGraph(min_weight)
        np.testing.assert_array_equal(G["frame_ids"], ids)
        want = {}
        for k, f in enumerate(ids):
            if k:
                want[(ids[k - 1], f)] = 0
        for f in ids:
            for g, w in _conn(M, f).items():
                if w >= min_weight:
                    key = (min(f, g), max(f, g))
                    want[key] = max(want.get(key, 0), w)
        keys = sorted(want)
        assert [(ids[i], ids[j]) for i, j in zip(G["edge_i"], G["edge_j"])] == keys
        assert list(G["edge_weight"]) == [want[k] for k in keys]
        for n, (a, b) in enumerate(keys):
            Z = np.linalg.inv(poses[a]) @ poses[b]
            np.testing.assert_allclose(pgo_ref.qmat(G["edge_q"][n]), Z[:3, :3], atol=1e-14)
            np.testing.assert_allclose(G["edge_p"][n], Z[:3, 3], atol=1e-14)
        for n, f in enumerate(ids):
            np.testing.assert_allclose(pgo_ref.qmat(G["pose_q"][n]), poses[f][:3, :3], atol=1e-14)
            np.testing.assert_array_equal(G["pose_p"][n], poses[f][:3, 3])
    assert len(M.PoseGraph(1000)["edge_i"]) == 4 and len(M.PoseGraph(1)["edge_i"]) > 4
    # the graph of the map is a problem the solver takes: the measurements are consistent, the cost is zero
    G = M.PoseGraph(1)
    fx = np.zeros(5, np.uint8)
    fx[0] = 1
    out = pkg.pgo_host(G["pose_q"], G["pose_p"], fx, G["edge_i"], G["edge_j"], G["edge_q"], G["edge_p"],
                       np.ones((len(G["edge_i"]), 2)))
    assert out["cost_initial"] < 1e-26


def test_map_apply_pose_graph_against_restatement(pkg, small_map):
    M, ids, poses, sees, X = small_map
    L0 = np.array([0.3, -0.2, 0.5, 0.0, 0.6, 0.8])
    M.InsertMapline(7, L0)
    M.InsertMapline(9, L0)
    M.AddLineObservation(9, 20, 0)
    moved = [8, 20]
    new = {8: _T(-0.3, [4.0, 0.0, 1.0]), 20: _T(1.0, [0.0, 5.0, 0.5])}
    q = [pgo_ref.qexp(np.array([0.0, 0.0, y])) for y in (-0.3, 1.0)]
    M.ApplyPoseGraph(moved, q, [new[f][:3, 3] for f in moved])
    for f in ids:
        np.testing.assert_allclose(M.GetPose(f), new.get(f, poses[f]), atol=1e-15)
    for j in range(10):
        obs = sorted(f for f in moved if j in sees[f])
        want = X[j]
        if obs:
            D = new[obs[0]] @ np.linalg.inv(poses[obs[0]])
            want = D[:3, :3] @ X[j] + D[:3, 3]
        got = M.GetMappoint(100 + j)[0]
        np.testing.assert_allclose(got, want, atol=1e-13)
        if not obs:
            np.testing.assert_array_equal(got, X[j])  # points 4 and 5 of frames 0 / 5 only stay where they are
    assert any(not [f for f in moved if j in sees[f]] for j in range(10))
    np.testing.assert_array_equal(M.GetMapline(7)[0], L0)  # a line nobody listed observes stays
    D = new[20] @ np.linalg.inv(poses[20])                 # Pluecker (w, d): d' = R d, w' = R w + t x d'
    d1 = D[:3, :3] @ L0[3:]
    np.testing.assert_allclose(M.GetMapline(9)[0], np.concatenate([D[:3, :3] @ L0[:3] + np.cross(D[:3, 3], d1), d1]),
                               atol=1e-13)
    with pytest.raises(pkg.capi.RsplError, match=r"rc=-1"):
        M.ApplyPoseGraph([3, 4], q[:2], [[0, 0, 0]] * 2)
    with pytest.raises(pkg.capi.RsplError, match=r"rc=-1"):
        M.ApplyPoseGraph([3, 3], q[:2], [[0, 0, 0]] * 2)
    np.testing.assert_array_equal(M.GetPose(3), poses[3])  # a refused call changes nothing


def test_map_loop_candidates_against_restatement(pkg, small_map):
    M, ids, poses, sees, X = small_map
    pts = [100, 101, 102, 103, 104, 105, -1, 999, 110]
    for frame, gap in ((20, 0), (20, 12), (8, 0), (0, 3)):
        votes = {}
        conn = _conn(M, frame)
        for pid in pts:
            for f in ids:
                if pid - 100 in sees[f] and f != frame and f not in conn and abs(f - frame) > gap:
                    votes[f] = votes.get(f, 0) + 1
        want = sorted(votes.items(), key=lambda kv: (-kv[1], kv[0]))
        got_ids, got_votes = M.LoopCandidates(frame, pts, gap)
        assert list(zip(got_ids, got_votes)) == want, (frame, gap)
    with pytest.raises(pkg.capi.RsplError, match=r"rc=-1"):
        M.LoopCandidates(4, pts, 0)
