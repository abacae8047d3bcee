"""CPU-side checks of relocalisation (rspl_lmap_global_*, rspl_map_good_mappoints, api.Relocalise): the boundary is
declared and bound; rspl_lmap_debug_global_host -- the contract on host arrays, distances in the fixed summation
order -- equals the numpy restatement (tests/reloc_ref.py) bit for bit on every case the GPU tests run; the designed
ties and threshold cases decide as designed; the map walk skips what is not Good; Relocalise's gates on stubbed
counts.  No GPU needed.

Parity is with this project's restatement: the reference has no relocalisation."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest

import reloc_cases as RC
import reloc_ref as RR

ROOT = pathlib.Path(__file__).resolve().parents[1]
FUNCS = ("rspl_lmap_global_enqueue", "rspl_lmap_global_fetch", "rspl_lmap_debug_global_host",
         "rspl_lmap_debug_global_plan", "rspl_map_good_mappoints")
INT_KEYS = ("n_keypoints", "n_local", "n_pass", "n_matched", "arg", "match", "kbest", "match_kp", "match_local",
            "match_id")
BIT_KEYS = ("best", "second", "match_pos", "match_xy")


@pytest.fixture(scope="module")
def pkg():
    import rspl_loader
    return rspl_loader.load()


def same_bits(got, want):
    assert set(got) == set(want)
    for k in INT_KEYS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    for k in BIT_KEYS:  # doubles compared as integers
        np.testing.assert_array_equal(np.ascontiguousarray(got[k]).view(np.int64),
                                      np.ascontiguousarray(want[k]).view(np.int64), err_msg=k)


def host(pkg, F, lm, **kw):
    return pkg.lmap_global_host(F, lm["ids"], lm["pos"], lm["desc"], **kw)


# 1: the boundary -----------------------------------------------------------------------------------------------
def test_header_declares_global_api_and_keeps_abi_2():
    hdr = (ROOT / "include" / "rspl.h").read_text()
    names = set(re.findall(r"\b(rspl_[a-z0-9_]+)\s*\(", hdr))
    for n in FUNCS:
        assert n in names
    for s in ("rspl_lmap_global_params", "rspl_lmap_global_result", "rspl_lmap_global_host_problem"):
        assert re.search(r"}\s*%s;" % s, hdr), s
    assert "#define RSPL_ABI_VERSION 2" in hdr  # no existing struct changed


def test_capi_binds_global_api(pkg):
    lib = pkg.capi.load()
    for n in FUNCS:
        assert n in pkg.capi.EXPORTS and hasattr(lib, n)
    assert [f[0] for f in pkg.capi.LmapGlobalParams._fields_] == ["max_distance", "max_ratio", "mutual"]
    assert len(lib.rspl_lmap_global_enqueue.argtypes) == 5
    for n in ("lmap_global_host", "lmap_global_plan", "Relocalise"):
        assert callable(getattr(pkg, n))


def test_plan(pkg):
    c, q, k = pkg.lmap_global_plan(256, 1024)
    assert c % 16 == 0 and q % 16 == 0 and 256 % k == 0 and k % 4 == 0
    c2 = pkg.lmap_global_plan(1024, 8320)[0]
    assert c2 > c and c2 % c == 0  # a larger table folds more bank rows into one workgroup
    with pytest.raises(pkg.capi.RsplError, match="capacities"):
        pkg.lmap_global_plan(0, 5)


# 2: the host twin equals the restatement bit for bit -------------------------------------------------------------
def plan_sizes(pkg):
    c, q, _ = pkg.lmap_global_plan(256, 1024)
    return RC.sizes(c, q)


def test_host_equals_ref_bitwise_on_every_size(pkg):
    for n1, nl in plan_sizes(pkg) + [(130, 1025)]:
        F, lm = RC.random_case(n1, nl, seed=100 * n1 + nl)
        for mutual in (True, False):
            same_bits(host(pkg, F, lm, mutual=mutual), RR.search(F, lm, mutual=mutual))


def test_ref_distance_is_the_plain_one():
    F, lm = RC.random_case(17, 65, seed=3)
    D = RR.distances(F, lm)
    np.testing.assert_allclose(D, 2.0 * (1.0 - F[:, 3:] @ lm["desc"].T), atol=1e-13, rtol=0)
    r = RR.search(F, lm, D=D)
    two = np.sort(D, axis=1)[:, :2]
    np.testing.assert_array_equal(r["best"], two[:, 0])
    np.testing.assert_array_equal(r["second"], two[:, 1])
    np.testing.assert_array_equal(r["arg"], np.argmin(D, axis=1))
    assert 5 < r["n_matched"] <= r["n_pass"] < 17


# 3: designed cases -----------------------------------------------------------------------------------------------
def test_duplicate_bank_rows(pkg):
    c = pkg.lmap_global_plan(256, 1024)[0]
    F, lm, want = RC.duplicate_bank_rows(c)
    r = host(pkg, F, lm)
    same_bits(r, RR.search(F, lm))
    for k, a in want:
        assert r["arg"][k] == a and r["second"][k] == r["best"][k] < 0.35 and r["match"][k] == -1


def test_duplicate_keypoints(pkg):
    q = pkg.lmap_global_plan(256, 1024)[1]
    F, lm, want = RC.duplicate_keypoints(q)
    r = host(pkg, F, lm)
    same_bits(r, RR.search(F, lm))
    for a, b, p in want:
        assert r["kbest"][p] == a and r["match"][a] == p and r["match"][b] == -1
    same_bits(host(pkg, F, lm, mutual=False), RR.search(F, lm, mutual=False))


def test_thresholds(pkg):
    F, lm, want = RC.thresholds()
    r = host(pkg, F, lm)
    same_bits(r, RR.search(F, lm))
    assert [bool(m >= 0) for m in r["match"][:4]] == want
    assert abs(r["best"][0] - 0.35) < 2e-6 and abs(r["best"][1] - 0.35) < 2e-6
    # the thresholds are the call's: moved across the same distances, the decisions swap
    r2 = host(pkg, F, lm, max_distance=0.35 + 2e-6, max_ratio=0.6 - 1e-5)
    same_bits(r2, RR.search(F, lm, max_distance=0.35 + 2e-6, max_ratio=0.6 - 1e-5))
    assert [bool(m >= 0) for m in r2["match"][:4]] == [True, True, False, False]


def test_mutual_differs(pkg):
    F, lm = RC.mutual_differs()
    r1, r0 = host(pkg, F, lm, mutual=True), host(pkg, F, lm, mutual=False)
    same_bits(r1, RR.search(F, lm, mutual=True))
    same_bits(r0, RR.search(F, lm, mutual=False))
    assert list(r1["match"][:2]) == [-1, 6] and list(r0["match"][:2]) == [6, 6]
    assert list(r0["match_kp"][:2]) == [0, 1] and list(r0["match_id"][:2]) == [lm["ids"][6]] * 2


def test_empty_operands(pkg):
    F, lm = RC.random_case(5, 7, seed=9)
    none = dict(ids=lm["ids"][:0], pos=lm["pos"][:0], desc=lm["desc"][:0])
    r = host(pkg, F, none)
    same_bits(r, RR.search(F, none))
    assert (r["arg"] == -1).all() and (r["best"] == 4.0).all() and (r["second"] == 4.0).all() and r["n_matched"] == 0
    r = host(pkg, F[:0], lm)
    same_bits(r, RR.search(F[:0], lm))
    assert (r["kbest"] == -1).all() and len(r["arg"]) == 0 and r["n_pass"] == 0
    one = dict(ids=lm["ids"][:1], pos=lm["pos"][:1], desc=lm["desc"][:1])
    r = host(pkg, F, one)
    same_bits(r, RR.search(F, one))
    assert (r["arg"] == 0).all() and (r["second"] == 4.0).all()


# 4: the map walk -------------------------------------------------------------------------------------------------
def test_good_mappoints(pkg):
    from test_lmap_cpu import _graph
    m, g = _graph(pkg)
    ids, pos = m.GoodMappoints()
    want = sorted(i for i, p in g["points"].items() if p["type"] == 1)
    assert list(ids) == want and 5 not in want and 21 not in want and len(want) == 40  # bad / untriangulated skipped
    np.testing.assert_array_equal(pos, np.array([g["points"][i]["p"] for i in want]))
    n, buf = C.c_int(), np.full(10, -7, np.int32)
    rc = pkg.capi.load().rspl_map_good_mappoints(m._h, buf.ctypes.data, None, 10, C.byref(n))
    assert rc == -4 and n.value == 40 and (buf == -7).all()  # RSPL_E_CAPACITY: the count, nothing written
    with pytest.raises(pkg.capi.RsplError, match="capacity 10"):
        m.GoodMappoints(cap=10)
    ids2, _ = m.GoodMappoints(cap=64)
    assert list(ids2) == want


def test_host_check_program():
    """tests/c/reloc_check.cpp: the host walk from C++ on exact descriptors, linked with the library's own objects
    (tests/c/reloc_check.mk; `reloc_check_san` there is the same program under ASan + UBSan)"""
    import subprocess
    subprocess.run(["make", "-C", str(ROOT / "tests" / "c"), "-f", "reloc_check.mk", "reloc_check"], check=True,
                   capture_output=True)
    r = subprocess.run([str(ROOT / "tests" / "c" / "build" / "reloc_check")], capture_output=True, text=True)
    assert r.returncode == 0 and "reloc_check: ok" in r.stdout, r.stdout + r.stderr


# 5: Relocalise's gates on stubbed counts -------------------------------------------------------------------------
class _StubLocalMap:
    def __init__(self, n_matched):
        self.n, self.calls = n_matched, []

    def set_local(self, ids, pos, stream=None):
        self.calls.append(("set_local", len(ids)))

    def global_enqueue(self, frames, stream=None, **kw):
        self.calls.append(("global_enqueue", len(frames)))

    def global_fetch(self):
        return [dict(n_matched=self.n, n_pass=self.n, match_pos=np.zeros((self.n, 3)), match_xy=np.zeros((self.n, 2)))]


class _StubPnP:
    def __init__(self, k):
        self.k, self.args = k, None

    def solve(self, frames, iterations, reprojection_error, confidence):
        self.args = (len(frames[0][1]), iterations, reprojection_error, confidence)
        T = np.eye(3)
        return [(self.k, T, np.array([1.0, 2.0, 3.0]), np.ones(self.args[0], np.uint8), 1)]


class _StubMap:
    def GoodMappoints(self):
        return np.arange(4, dtype=np.int32), np.zeros((4, 3))


def test_relocalise_gates(pkg, monkeypatch):
    from rspl_slam_amd import api
    frame = dict(cam=(400.0, 400.0, 320.0, 240.0, 40.0), Twc=np.eye(4))
    seen = {}

    def fake_track(map_, lm, tracker, fr, ref, min_num_match, num_inlier_thr, stream):
        seen.update(Twc=fr["Twc"], last=fr["last_Twc"], ref=ref)
        return 42, dict(n_good=50)

    monkeypatch.setattr(api, "TrackLocalMap", fake_track)
    # the search gate: max(8, min_num_match) matches
    for n, mnm, stage in ((7, 3, "search"), (9, 10, "search"), (8, 3, "pnp")):
        lm, pnp = _StubLocalMap(n), _StubPnP(2)
        r, info = api.Relocalise(None, lm, None, pnp, frame, min_num_match=mnm)
        assert r == -1 and info["stage"] == stage and info["n_matched"] == n
        assert (pnp.args is None) == (stage == "search") and not seen
    # the PnP gate: n_inliers < min_num_match; the reference's 100 / 20 px / 0.99
    lm, pnp = _StubLocalMap(30), _StubPnP(9)
    r, info = api.Relocalise(None, lm, None, pnp, frame)
    assert r == -1 and info["stage"] == "pnp" and info["pnp_inliers"] == 9 and pnp.args == (30, 100, 20.0, 0.99)
    # through: the chain starts from PnP's pose, which is also the last pose of the 0.5 m gate
    lm, pnp = _StubLocalMap(30), _StubPnP(10)
    r, out = api.Relocalise(_StubMap(), lm, None, pnp, frame, candidates="map", ref_keyframe=3)
    assert r == 42 and out["stage"] == "track" and out["n_good"] == 50 and out["pnp_inliers"] == 10
    assert lm.calls == [("set_local", 4), ("global_enqueue", 1)] and seen["ref"] == 3
    np.testing.assert_array_equal(seen["Twc"][:3, 3], [1.0, 2.0, 3.0])
    assert seen["last"] is seen["Twc"]
    lm = _StubLocalMap(30)
    api.Relocalise(None, lm, None, _StubPnP(10), frame, candidates=(np.arange(6), np.zeros((6, 3))))
    assert lm.calls[0] == ("set_local", 6)
    with pytest.raises(ValueError):
        api.Relocalise(None, lm, None, pnp, frame, candidates="all")
