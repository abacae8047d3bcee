"""Relocalisation on the device (rspl_lmap_global_*, api.Relocalise) against rspl_lmap_debug_global_host, the host
twin that tests/test_reloc_cpu.py pins to the numpy restatement bit for bit.  The device evaluates the distances on
fp64 MFMA in another summation order, so:

  decisions (arg, kbest, match, the counts, the compacted match list) are compared EXACTLY -- every generated case
  asserts on the CPU that no decision sits within 1e-9 of its threshold, and the designed ties are between identical
  bits, which the device must turn into identical distances whatever tile they land in;

  best / second are held to 1e-13 absolute: a length-256 dot product of unit vectors errs by at most
  gamma_256 ~ 256 * 2^-53 ~ 2.85e-14 in any order, doubled by 2 (1 - dot), plus the roundings after it and the
  host's own smaller error: ~6e-14.  Measured maximum over this file: see DESIGN section 5g.

Parity is with this project's restatement: the reference has no relocalisation."""
import numpy as np
import pytest

import lmap_cases as LC
import reloc_cases as RC
from conftest import pkg
from rspl_slam_amd import capi

pytestmark = pytest.mark.gpu

K, L, B = 256, 1024, 3
TOL = 1e-13
INT_KEYS = ("n_keypoints", "n_local", "n_pass", "n_matched", "arg", "match", "kbest", "match_kp", "match_local",
            "match_id")
C_ROWS, Q_ROWS, _ = pkg.lmap_global_plan(K, L)
worst = [0.0]


@pytest.fixture(scope="module")
def handle():
    return pkg.LocalMap(max_bank_points=L + 64, max_local_points=L, max_keypoints=K, max_batch=B)


def _dev(a):
    a = np.ascontiguousarray(a)
    b = capi.DeviceBuffer(max(a.nbytes, 8))
    if a.nbytes:
        b.upload(a)
    return b


def _frame(F, n1=None):
    return dict(d_features=_dev(F), d_n1=_dev(np.array([len(F) if n1 is None else n1], np.int32)))


def _compare(got, want):
    assert set(got) == set(want)
    for k in INT_KEYS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    np.testing.assert_array_equal(got["match_pos"], want["match_pos"])  # copies: exact
    np.testing.assert_array_equal(got["match_xy"], want["match_xy"])
    for k in ("best", "second"):
        if len(want[k]):
            d = float(np.abs(got[k] - want[k]).max())
            worst[0] = max(worst[0], d)
            print(f"max |d {k}| = {d:.3e} (running maximum {worst[0]:.3e})")
            assert d <= TOL, (k, d)


def _check(h, Fs, lm, **kw):
    """one global enqueue of the frames `Fs` against the table `lm`"""
    h.store_host(lm["ids"], lm["desc"])
    h.set_local(lm["ids"], lm["pos"])
    dev = [_frame(F) for F in Fs]
    h.global_enqueue(dev, **kw)
    res = h.global_fetch()
    assert len(res) == len(Fs)
    for F, r in zip(Fs, res):
        _compare(r, pkg.lmap_global_host(F[:h.max_keypoints], lm["ids"], lm["pos"], lm["desc"], **kw))
    return res


@pytest.mark.parametrize("n1,nl", RC.sizes(C_ROWS, Q_ROWS))
def test_size_boundaries(handle, n1, nl):
    F, lm = RC.random_case(n1, nl, seed=100 * n1 + nl)
    (r,) = _check(handle, [F], lm)
    assert (r["n_keypoints"], r["n_local"]) == (n1, nl)
    if min(n1, nl) >= 15:
        assert r["n_matched"] > 3
    _check(handle, [F], lm, mutual=False)


def test_chunk_of_several_groups():
    """a handle whose plan folds more than one 64-row group into a workgroup: the per-keypoint state carried across
    the groups of a chunk, the per-point partial written per group"""
    c, q, _ = pkg.lmap_global_plan(1024, 8320)
    assert c > C_ROWS
    h = pkg.LocalMap(max_bank_points=8320, max_local_points=8320, max_keypoints=1024, max_batch=1)
    for nl in (c - 1, c, c + 1, 2 * c + 1):
        F, lm = RC.random_case(q + 1, nl, seed=7000 + nl)
        _check(h, [F], lm)


def test_batch_of_three(handle):
    """three frames with different counts, one of them empty, against one table; then a batch of one leaks nothing"""
    F, lm = RC.random_case(130, 200, seed=130200)
    Fs = [F, F[:0], F[40:57]]
    res = _check(handle, Fs, lm)
    assert [r["n_keypoints"] for r in res] == [130, 0, 17] and (res[1]["kbest"] == -1).all()
    one = _check(handle, Fs[2:], lm)
    for k in one[0]:
        np.testing.assert_array_equal(one[0][k], res[2][k], err_msg=k)


def test_permuted_subset_of_the_bank(handle):
    """the table is a permuted subset of the bank: the search gathers its rows through local_row"""
    F, lm = RC.random_case(65, 300, seed=65300)
    handle.store_host(lm["ids"][::-1], lm["desc"][::-1])  # bank rows in another order than any table
    pick = np.random.default_rng(5).permutation(300)[:150]
    sub = dict(ids=lm["ids"][pick], pos=lm["pos"][pick], desc=lm["desc"][pick])
    assert RC.RR.margins(F, sub) > LC.MARGIN
    handle.set_local(sub["ids"], sub["pos"])
    handle.global_enqueue([_frame(F)])
    (r,) = handle.global_fetch()
    _compare(r, pkg.lmap_global_host(F, sub["ids"], sub["pos"], sub["desc"]))
    assert r["n_matched"] > 3 and set(r["match_id"]) <= set(sub["ids"])


def test_keypoint_count_above_the_handles_capacity():
    """*d_n1 = 300 > max_keypoints = 256: the search works on the first 256 keypoints and reports 256"""
    F, lm = RC.random_case(300, 65, seed=30065)
    assert RC.RR.margins(F[:K], lm) > LC.MARGIN
    h = pkg.LocalMap(max_bank_points=128, max_local_points=128, max_keypoints=K, max_batch=1)
    (r,) = _check(h, [F], lm)
    assert r["n_keypoints"] == K and len(r["arg"]) == K


def test_duplicate_bank_rows(handle):
    F, lm, want = RC.duplicate_bank_rows(C_ROWS)
    (r,) = _check(handle, [F], lm)
    for k, a in want:  # identical bits, identical distances: inside a tile, across the chunk boundary, in the tail
        assert r["arg"][k] == a and r["second"][k] == r["best"][k] and r["match"][k] == -1


def test_duplicate_keypoints(handle):
    F, lm, want = RC.duplicate_keypoints(Q_ROWS)
    (r,) = _check(handle, [F], lm)
    for a, b, p in want:
        assert r["kbest"][p] == a and r["match"][a] == p and r["match"][b] == -1 and r["best"][a] == r["best"][b]
    (r0,) = _check(handle, [F], lm, mutual=False)
    assert all(r0["match"][b] == p for _, b, p in want)


def test_thresholds_and_mutual(handle):
    F, lm, want = RC.thresholds()
    (r,) = _check(handle, [F], lm)
    assert [bool(m >= 0) for m in r["match"][:4]] == want
    (r2,) = _check(handle, [F], lm, max_distance=0.35 + 2e-6, max_ratio=0.6 - 1e-5)
    assert [bool(m >= 0) for m in r2["match"][:4]] == [True, True, False, False]
    F, lm = RC.mutual_differs()
    (r1,), (r0,) = _check(handle, [F], lm, mutual=True), _check(handle, [F], lm, mutual=False)
    assert list(r1["match"][:2]) == [-1, 6] and list(r0["match"][:2]) == [6, 6]


# ---- end to end -------------------------------------------------------------------------------------------------
def _lmap_frame(fr):
    n1 = len(fr["features"])
    return dict(d_features=_dev(fr["features"]), d_n1=_dev(np.array([n1], np.int32)), d_point_id=_dev(fr["point_id"]),
                d_point_xyz=_dev(fr["point_xyz"]), Twc=fr["Twc"], cam=fr["cam"], width=fr["width"], height=fr["height"])


def test_relocalise_end_to_end():
    """a pose 3 m and 0.6 rad away: the local-map chain alone fails, Relocalise finds the ground truth to the 1e-9
    that tests/test_gpu_lmap.py holds the chain to on this noise-free scene; with unrelated candidate descriptors it
    stops at the search"""
    from rspl_slam_amd import synthetic as SY
    fr, lm, gt, stale = RC.reloc_scene()
    assert np.linalg.norm(stale[:3, 3] - gt[:3, 3]) == pytest.approx(3.0) and 200 <= len(lm["ids"]) <= 256
    h = pkg.LocalMap(max_bank_points=512, max_local_points=256, max_keypoints=K, max_batch=1)
    h.store_host(lm["ids"], lm["desc"])
    h.set_local(lm["ids"], lm["pos"])
    t = pkg.Tracker(max_batch=1, max_keypoints=K)
    pnp = pkg.PnP(max_batch=1, max_points=K)
    d = _lmap_frame(fr)
    assert pkg.TrackLocalMap(None, h, t, d)[0] == -1  # the precondition: the stale pose cannot be tracked from
    n, out = pkg.Relocalise(None, h, t, pnp, d, candidates=(lm["ids"], lm["pos"]))
    assert out["stage"] == "track" and n > 10 and out["n_matched"] >= 190 and out["pnp_inliers"] >= 190
    assert np.abs(out["pose_p"] - gt[:3, 3]).max() < 1e-9
    assert np.abs(SY.quat_xyzw_to_R(out["pose_q"]) - gt[:3, :3]).max() < 1e-9
    # every candidate descriptor replaced by an unrelated one
    h2 = pkg.LocalMap(max_bank_points=512, max_local_points=256, max_keypoints=K, max_batch=1)
    h2.store_host(lm["ids"], LC.unit(np.random.default_rng(99), len(lm["ids"])))
    n2, info = pkg.Relocalise(None, h2, t, pnp, d, candidates=(lm["ids"], lm["pos"]))
    assert n2 == -1 and info["stage"] == "search" and info["n_matched"] < 8


def test_enqueue_contract(handle):
    F, lm = RC.random_case(5, 3, seed=1)
    handle.store_host(lm["ids"], lm["desc"])
    handle.set_local(lm["ids"], lm["pos"])
    fr, lmp = LC.random_scene(5, 1, seed=1)
    proj = _lmap_frame(fr)
    g = _frame(F)
    with pytest.raises(capi.RsplError, match="NULL device pointer"):  # before any launch
        handle.global_enqueue([dict(g, d_features=None)])
    with pytest.raises(capi.RsplError, match="exceeds max_batch"):
        handle.global_enqueue([g] * (B + 1))
    handle.enqueue([proj])  # a projection enqueue unfetched: the global one is refused, and the other way round
    with pytest.raises(capi.RsplError, match="has not been fetched"):
        handle.global_enqueue([g])
    handle.fetch()
    handle.global_enqueue([g])
    with pytest.raises(capi.RsplError, match="has not been fetched"):
        handle.enqueue([proj])
    with pytest.raises(capi.RsplError, match="in flight"):
        handle.set_local(lm["ids"], lm["pos"])
    with pytest.raises(capi.RsplError, match="is a global one"):
        handle.fetch()
    (r,) = handle.global_fetch()
    assert r["n_keypoints"] == 5 and r["n_local"] == 3
    handle.global_enqueue([])
    assert handle.global_fetch() == []
    host_only = pkg.LocalMap(max_bank_points=8, max_local_points=8, max_keypoints=8, max_batch=1, device=-1)
    with pytest.raises(capi.RsplError, match="host-only"):
        host_only.global_enqueue([g])
