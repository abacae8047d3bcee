"""The part of a local BA call that is not an LM trial: the Schur chunks' edge-pair lists filled by the first
pass against the offsets the host staging counted, and the final kernel's 16-byte stores through the inverse edge
map.  Windows of tests/ba_frame_cases.py (the 64-lane rounds and the 256-landmark range edge, landmarks of 9 and 17
edges, several edges on one pose, inactive landmarks, a second fixed pose, empty chunks, lines only, diagonal
sub-chunks, a shuffled caller order).  Everything here is exact: integers, flags and copied doubles."""
import ctypes as C

import numpy as np
import pytest

from rspl_slam_amd import capi

import ba_frame_cases as BC

pytestmark = pytest.mark.gpu

CASES = BC.structure_cases()
IDS = [n for n, _ in CASES]


@pytest.fixture(scope="module")
def ba():
    import rspl_loader
    return rspl_loader.load().LocalBA(**BC.CAPS)


def _staged_offsets(p):
    cap = 1 << 16
    off, nc = np.zeros(cap, np.int32), C.c_int()
    P = p.to_ctypes()
    capi.check(capi.load().rspl_ba_debug_pair_offsets(C.byref(P), BC.MAX_LANDMARKS, BC.CAPS["max_poses"],
                                                      off.ctypes.data, cap, C.byref(nc)), "rspl_ba_debug_pair_offsets")
    return off[:nc.value + 1]


def _submit(ba, p):
    """the call through the handle's tracking / staging threads (rspl_ba_submit): staged off the device's chain, so
    the staging counts the edge-pair offsets"""
    r = ba.submit(p)
    ba.join()
    return r


def _same_result(a, b):
    np.testing.assert_array_equal(a.pose_q, b.pose_q)
    np.testing.assert_array_equal(a.pose_p, b.pose_p)
    np.testing.assert_array_equal(a.points, b.points)
    np.testing.assert_array_equal(a.lines, b.lines)
    for k, _ in BC.KINDS:
        np.testing.assert_array_equal(a.inlier[k], b.inlier[k], err_msg=k)
    assert (a.chi2_first, a.iters_first, a.chi2_second, a.iters_second) == \
        (b.chi2_first, b.iters_first, b.chi2_second, b.iters_second)


@pytest.mark.parametrize("name,p", CASES, ids=IDS)
def test_fused_pair_lists_equal_build_pairs(ba, name, p):
    """the lists a submitted call's first pass filled against the staged offsets == the count / scan / fill
    launches' on the same structure, element by element; the offsets == the host staging's; a synchronous call
    (rspl_ba_local: counted in the first pass on the device) builds the same lists"""
    _submit(ba, p)
    off_f, pp_f, staged = ba.debug_pairs()
    assert staged  # (every case is inside the device LM driver's windows)
    off_b, pp_b, _ = ba.debug_pairs(rebuild=True)
    np.testing.assert_array_equal(off_f, off_b)
    np.testing.assert_array_equal(off_f, _staged_offsets(p))
    assert pp_f.shape[0] == off_f[-1]
    np.testing.assert_array_equal(pp_f, pp_b)
    ba.run(p)
    off_s, pp_s, staged = ba.debug_pairs()
    assert not staged
    np.testing.assert_array_equal(off_s, off_f)
    np.testing.assert_array_equal(pp_s, pp_f)


@pytest.mark.parametrize("name,p", CASES, ids=IDS)
def test_fused_call_equals_host_ordered_call(ba, name, p):
    """a submitted call (staged offsets; final kernel and the second optimize's setup queued speculatively) and the
    same call made synchronously against the host-ordered launches taken with kernel timing: bit-identical results"""
    spec = _submit(ba, p)
    _same_result(spec, ba.run(p))
    ba.kernel_timing(1)
    try:
        host = ba.run(p)
    finally:
        ba.kernel_timing(0)
        ba.kernel_times()
    _same_result(spec, host)


@pytest.fixture(scope="module")
def flag_base():
    p = BC.window(70, 4, seed=21, n_lines=8)
    assert all(p.n_edges(k) >= 3 for k, _ in BC.KINDS), [p.n_edges(k) for k, _ in BC.KINDS]
    return p


@pytest.mark.parametrize("how", ["submitted", "speculative", "host-ordered"])
@pytest.mark.parametrize("E", [1, 15, 16, 17, 255, 257])
def test_final_kernel_equals_classify_path(ba, flag_base, E, how):
    """the final kernel's flags (the caller's order, 16 per store) and T / X / L against the classify kernel's final
    pass carried through gmap and the device state, for edge counts around the 16-byte words and the 256-flag
    blocks, all four edge types, the caller's order shuffled"""
    p = BC.with_total_edges(flag_base, E, np.random.default_rng(E))
    assert BC.n_edges(p) == E
    if E >= 4:
        assert all(p.n_edges(k) >= 1 for k, _ in BC.KINDS)
    ba.kernel_timing(1 if how == "host-ordered" else 0)
    try:
        r = _submit(ba, p) if how == "submitted" else ba.run(p)
        d = ba.debug_final(p)
    finally:
        ba.kernel_timing(0)
        ba.kernel_times()
    got = np.concatenate([r.inlier[k].astype(np.uint8).reshape(-1) for k, _ in BC.KINDS])
    assert got.shape[0] == E and set(np.unique(d["inlier"])) <= {0, 1}
    np.testing.assert_array_equal(got, d["inlier"])
    np.testing.assert_array_equal(d["T_out"], d["T_dev"])
    np.testing.assert_array_equal(r.points, d["points"])
    np.testing.assert_array_equal(r.lines, d["lines"])
    if E >= 255:
        assert 0 < got.sum()  # (some inliers: the flags are not one constant)
