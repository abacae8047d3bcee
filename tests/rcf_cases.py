"""The RCF test cases shared by tests/test_rcf_cpu.py and tests/test_gpu_rcf.py: (H, W, seed) of
rcf_ref.test_image under weights.rcf_synth(7)."""
import pathlib

ROOT = pathlib.Path(__file__).resolve().parents[1]

# 16 x 16: the smallest size; 17 x 33: one past a tile edge in both axes; 37 x 51: odd at every pooling level;
# 64 x 80: whole tiles
SINGLE = [(16, 16, 0), (17, 33, 0), (37, 51, 0), (64, 80, 0)]
BATCH = [(40, 56, 0), (40, 56, 1), (40, 56, 2)]  # one call of three images, padded strides and pitches
ALL = SINGLE + BATCH


def rcf_blob():
    from rspl_slam_amd import weights as WT
    return WT.ensure_rcf_blob(str(ROOT / "weights"))
