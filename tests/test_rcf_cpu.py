"""CPU-side checks of the RCF edge network (rspl_rcf_*, rspl_slam_amd.RCF): the boundary is declared and bound,
the synthetic weights round-trip through the blob with the state_dict's names and shapes, bad configurations
and blobs are refused before a device is touched, the restatement (tests/rcf_ref.py) lands on H x W at every
stage for odd and even sizes, and every GPU test case spreads its edge image over the transfer curve."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest

import rcf_ref as RR
from rcf_cases import ALL

ROOT = pathlib.Path(__file__).resolve().parents[1]
FUNCS = ("rspl_rcf_debug_sizeof", "rspl_rcf_create", "rspl_rcf_destroy", "rspl_rcf_infer", "rspl_rcf_infer_device",
         "rspl_rcf_debug_logits", "rspl_rcf_debug_tile_rows", "rspl_rcf_profile",
         "rspl_rcf_stage_times")


def _capi():
    import rspl_loader
    return rspl_loader.load().capi


def test_header_declares_rcf_api():
    hdr = (ROOT / "include" / "rspl.h").read_text()
    names = set(re.findall(r"\b(rspl_[a-z0-9_]+)\s*\(", hdr))
    for n in FUNCS:
        assert n in names
    assert re.search(r"}\s*rspl_rcf_config;", hdr)
    assert "#define RSPL_ABI_VERSION 2" in hdr  # no existing struct changed


def test_capi_binds_rcf_api_and_struct_layout():
    capi = _capi()
    lib = capi.load()
    for n in FUNCS:
        assert n in capi.EXPORTS and hasattr(lib, n)
    assert len(lib.rspl_rcf_infer_device.argtypes) == 11 and len(lib.rspl_rcf_infer.argtypes) == 6
    assert [f[0] for f in capi.RcfConfig._fields_] == ["max_height", "max_width", "max_batch", "precision", "output",
                                                       "device"]
    assert lib.rspl_rcf_debug_sizeof(0) == C.sizeof(capi.RcfConfig) == 24
    assert lib.rspl_rcf_debug_sizeof(1) == -1


def test_shapes_are_the_state_dict():
    from rspl_slam_amd import weights as WT
    sh = WT.rcf_shapes()
    assert len(sh) == 2 * (13 + 13 + 5 + 1)
    assert sh["conv1_1.weight"] == (64, 3, 3, 3) and sh["conv1_2.weight"] == (64, 64, 3, 3)
    assert sh["conv2_1.weight"] == (128, 64, 3, 3) and sh["conv3_3.weight"] == (256, 256, 3, 3)
    assert sh["conv4_1.weight"] == (512, 256, 3, 3) and sh["conv5_3.weight"] == (512, 512, 3, 3)
    assert sh["conv3_2_down.weight"] == (21, 256, 1, 1) and sh["conv5_1_down.bias"] == (21,)
    assert sh["score_dsn4.weight"] == (1, 21, 1, 1) and sh["score_fuse.weight"] == (1, 5, 1, 1)
    assert "conv1_3.weight" not in sh and "conv3_3.weight" in sh and "conv3_4.weight" not in sh
    # VGG16's 13 convolutions (14 714 688 weights and biases with 3 input channels) and the side branches
    vgg = sum(int(np.prod(v)) for k, v in sh.items() if re.fullmatch(r"conv\d_\d\.(weight|bias)", k))
    assert vgg == 14714688
    w = RR.synth_weights()
    assert list(w) == list(sh) and all(w[k].shape == tuple(v) and w[k].dtype == np.float32 for k, v in sh.items())
    a1, a2 = np.sqrt(6.0 / 27), np.sqrt(6.0 / 576)
    assert 0.9 * 0.01 * a1 < np.abs(w["conv1_1.weight"]).max() <= 0.01 * a1  # the first layer's gain
    assert 0.9 * a2 < np.abs(w["conv1_2.weight"]).max() <= a2


def test_blob_round_trip(tmp_path):
    from rspl_slam_amd import weights as WT
    w = RR.synth_weights()
    WT.write_blob(tmp_path / "rcf.bin", w)
    back = WT.read_blob(tmp_path / "rcf.bin")
    assert list(back) == list(w)
    for k in w:
        assert back[k].shape == w[k].shape and back[k].tobytes() == w[k].tobytes(), k
    assert WT.rcf_synth(7)["conv4_2.weight"].tobytes() == w["conv4_2.weight"].tobytes()  # deterministic
    assert WT.rcf_synth(8)["conv4_2.weight"].tobytes() != w["conv4_2.weight"].tobytes()


def _create(capi, blob, **kw):
    cfg = dict(max_height=64, max_width=96, max_batch=2, precision=capi.RSPL_PREC_FP32, output=5, device=0)
    cfg.update(kw)
    c = capi.RcfConfig(*[cfg[f[0]] for f in capi.RcfConfig._fields_])
    h = C.c_void_p()
    rc = capi.load().rspl_rcf_create(C.byref(c), str(blob).encode(), C.byref(h))
    assert rc != 0 and not h.value
    return rc, capi.load().rspl_last_error().decode()


@pytest.mark.parametrize("bad", [dict(max_height=15), dict(max_width=8), dict(max_height=2049), dict(max_width=4096),
                                 dict(max_batch=0), dict(max_batch=65), dict(precision=2), dict(precision=-1),
                                 dict(output=6), dict(output=-1)])
def test_bad_config_is_refused_before_the_blob_and_the_device(tmp_path, bad):
    rc, msg = _create(_capi(), tmp_path / "absent.bin", **bad)
    assert rc == -1 and "rspl_rcf_create" in msg, (rc, msg)  # RSPL_E_ARG, not the missing file's RSPL_E_WEIGHTS


def test_bad_blob_is_refused_and_names_the_tensor(tmp_path):
    """A stripped-down state_dict (one value per output channel would not pass either): a missing tensor and a
    mis-shaped one are RSPL_E_WEIGHTS with the tensor's name, before a device is touched (this test runs
    without one)."""
    from rspl_slam_amd import weights as WT
    capi = _capi()
    rc, msg = _create(capi, tmp_path / "absent.bin")
    assert rc == -2
    w = dict(RR.synth_weights())
    gone = {k: v for k, v in w.items() if k != "conv3_2_down.bias"}
    WT.write_blob(tmp_path / "gone.bin", gone)
    rc, msg = _create(capi, tmp_path / "gone.bin")
    assert rc == -2 and "conv3_2_down.bias" in msg, (rc, msg)
    shaped = dict(w)
    shaped["conv5_1.weight"] = np.ascontiguousarray(w["conv5_1.weight"].reshape(512, 512, 9))  # same count
    WT.write_blob(tmp_path / "shaped.bin", shaped)
    rc, msg = _create(capi, tmp_path / "shaped.bin")
    assert rc == -2 and "conv5_1.weight" in msg and "512,512,3,3" in msg, (rc, msg)
    one = dict(w)
    one["conv1_1.weight"] = w["conv1_1.weight"][:, :1].copy()  # a one-channel first layer is not the state_dict
    WT.write_blob(tmp_path / "one.bin", one)
    rc, msg = _create(capi, tmp_path / "one.bin")
    assert rc == -2 and "conv1_1.weight" in msg, (rc, msg)


def test_restatement_lands_on_the_image_size():
    """Every stage's size follows the pools' ceil_mode arithmetic, every crop lies inside its upsampled map
    (asserted in forward too) and all six maps are H x W, for H, W in {16, 17, 31, 37, 51, 64}."""
    sizes = (16, 17, 31, 37, 51, 64)
    got = RR.run_child("shapes", [(H, W, 0) for H in sizes for W in sizes])
    for H in sizes:
        for W in sizes:
            assert got[f"{H}x{W}_logits"].tolist() == [6, H, W, 1]  # (the last: every value finite)
            stage, up = got[f"{H}x{W}_stage"].tolist(), got[f"{H}x{W}_up"].tolist()
            assert [tuple(s) for s in stage] == RR.stage_sizes(H, W)
            for (size, stride, off), (hs, ws), (hu, wu) in zip(RR.UP, stage, up):
                assert (hu, wu) == ((hs - 1) * stride + size, (ws - 1) * stride + size)
                assert off + H <= hu and off + W <= wu


def test_bilinear_kernels():
    k4 = RR.bilinear_kernel(4)
    np.testing.assert_array_equal(k4[0], np.array([0.25, 0.75, 0.75, 0.25]) * 0.25)
    for size, stride in ((4, 2), (8, 4), (16, 8)):
        k = RR.bilinear_kernel(size)
        assert k.shape == (size, size) and np.array_equal(k, k.T) and np.array_equal(k, k[::-1, ::-1])
        # a constant map is reproduced: the taps of every output phase sum to one
        for py in range(stride):
            for px in range(stride):
                assert k[py::stride, px::stride].shape == (2, 2) and k[py::stride, px::stride].sum() == 1.0


@pytest.mark.parametrize("case", ALL)
def test_cases_are_not_saturated(case):
    """The fused edge image of every GPU test case has at least 128 distinct levels in the float64 restatement:
    a saturated image (all 0 / 255) would pass any parity check."""
    H, W, seed = case
    edge = RR.edge_image(RR.reference(H, W, "float64", False, seed)["logits"][5])
    assert edge.shape == (H, W) and len(np.unique(edge)) >= 128, len(np.unique(edge))


def test_fp16_restatement_differs_and_stays_close():
    """fp16=True does round (it is not the fp32 network) and stays within fp16's reach of it"""
    a = RR.reference(37, 51, "float64", False)["logits"]
    b = RR.reference(37, 51, "float64", True)["logits"]
    d = np.abs(a - b).max()
    assert 1e-5 < d < 0.1, d
