"""Generators of the relocalisation tests (tests/test_reloc_cpu.py, tests/test_gpu_reloc.py): keypoint records and
candidate tables in tests/reloc_ref.py's format, built on lmap_cases.unit / at_distance.  A case that is not a
designed tie asserts here, on the CPU, that every decision margin of the restatement exceeds lmap_cases.MARGIN."""
import numpy as np

import lmap_cases as LC
import reloc_ref as RR

PARAMS = dict(max_distance=RR.MAX_DISTANCE, max_ratio=RR.MAX_RATIO, mutual=True)


def records(desc, rng):
    """[n, 259] records around the descriptors: score, x, y on quarter pixels"""
    desc = np.asarray(desc, np.float64).reshape(-1, 256)
    F = np.zeros((len(desc), 259))
    F[:, 0] = 0.5
    F[:, 1] = np.round(rng.uniform(1, 751, len(desc)) * 4) / 4
    F[:, 2] = np.round(rng.uniform(1, 479, len(desc)) * 4) / 4
    F[:, 3:] = desc
    return F


def table(desc, rng, first_id=100):
    desc = np.asarray(desc, np.float64).reshape(-1, 256)
    n = len(desc)
    return dict(ids=np.arange(first_id, first_id + n, dtype=np.int32), pos=rng.normal(0, 3, (n, 3)), desc=desc)


def checked(F, lm, **kw):
    m = RR.margins(F, lm, **kw)
    assert m > LC.MARGIN, f"a decision of this case sits {m} from its threshold"
    return F, lm


def random_case(n1, nl, seed):
    """a random unit bank; 75 % of the keypoints are a noisy copy, at distance U(0.02, 0.5), of a distinct bank row"""
    rng = np.random.default_rng(seed)
    bank = LC.unit(rng, nl).reshape(nl, 256)
    rows = rng.permutation(nl)
    q = []
    for i in range(n1):
        if i < nl and rng.uniform() < 0.75:
            q.append(LC.at_distance(bank[rows[i]], rng.uniform(0.02, 0.5), rng))
        else:
            q.append(LC.unit(rng))
    return checked(records(np.array(q).reshape(n1, 256), rng), table(bank, rng))


def sizes(c, q):
    """(keypoints, local points): the 16-row MFMA tile's edges, and the chunk (c) and query tile (q) boundaries"""
    out = [(k, l) for k in (0, 1, 15, 16, 17, 65) for l in (0, 1, 2, 15, 16, 17)]
    out += [(k, l) for l in (c - 1, c, c + 1, 2 * c + 1) for k in (q - 1, q, q + 1)]
    return out


# ---- designed cases ---------------------------------------------------------------------------------------------
def duplicate_bank_rows(c=64, seed=21):
    """three pairs of bank rows with identical bits -- inside a tile, across the chunk boundary, in the tail tile --
    each with one keypoint near it: arg is the lower row, second == best, the ratio test fails
    -> (F, lm, [(keypoint, lower row)])"""
    rng = np.random.default_rng(seed)
    nl = 2 * c + 5
    bank = LC.unit(rng, nl)
    pairs = [(3, 9), (c - 1, c), (2 * c + 1, 2 * c + 3)]
    for a, b in pairs:
        bank[b] = bank[a]
    q = LC.unit(rng, 20)
    want = []
    for k, (a, b) in zip((2, 11, 17), pairs):
        q[k] = LC.at_distance(bank[a], 0.1, rng)
        want.append((k, a))
    F, lm = records(q, rng), table(bank, rng)
    r = RR.search(F, lm)
    for k, a in want:
        assert r["arg"][k] == a and r["best"][k] == r["second"][k] and r["match"][k] == -1
    return F, lm, want


def duplicate_keypoints(q=64, seed=22):
    """three pairs of keypoints with identical bits -- inside a query tile, across its boundary, in the tail -- each
    near one bank row: kbest is the lower keypoint, and only that one is a mutual match
    -> (F, lm, [(lower keypoint, upper keypoint, row)])"""
    rng = np.random.default_rng(seed)
    n1 = q + 9
    bank = LC.unit(rng, 40)
    d = LC.unit(rng, n1)
    want = []
    for (a, b), p in zip([(2, 7), (q - 1, q), (q + 3, q + 8)], (5, 20, 33)):
        d[a] = LC.at_distance(bank[p], 0.1, rng)
        d[b] = d[a]
        want.append((a, b, p))
    F, lm = records(d, rng), table(bank, rng)
    r = RR.search(F, lm)
    for a, b, p in want:
        assert r["kbest"][p] == a and r["match"][a] == p and r["match"][b] == -1 and r["arg"][b] == p
    r0 = RR.search(F, lm, mutual=False)
    assert all(r0["match"][b] == p for _, b, p in want)
    return F, lm, want


def thresholds(seed=23):
    """best 1e-6 either side of max_distance, best / second 1e-6 either side of max_ratio
    -> (F, lm, expected pass per keypoint 0..3)"""
    rng = np.random.default_rng(seed)
    bank = LC.unit(rng, 30)
    q = LC.unit(rng, 8)
    q[0] = LC.at_distance(bank[0], 0.35 - 1e-6, rng)
    q[1] = LC.at_distance(bank[1], 0.35 + 1e-6, rng)
    q[2], q[3] = LC.unit(rng), LC.unit(rng)
    bank[2], bank[3] = LC.at_distance(q[2], 0.12, rng), LC.at_distance(q[2], 0.12 / 0.6 + 1e-6, rng)  # ratio just below
    bank[4], bank[5] = LC.at_distance(q[3], 0.12, rng), LC.at_distance(q[3], 0.12 / 0.6 - 1e-6, rng)  # ... just above
    F, lm = checked(records(q, rng), table(bank, rng))
    r = RR.search(F, lm)
    want = [True, False, True, False]
    assert [bool(m >= 0) for m in r["match"][:4]] == want and list(r["arg"][:4]) == [0, 1, 2, 4]
    return F, lm, want


def mutual_differs(seed=24):
    """keypoints 0 and 1 are both nearest to bank row 6, keypoint 1 closer: without the mutual test both match"""
    rng = np.random.default_rng(seed)
    bank = LC.unit(rng, 12)
    q = LC.unit(rng, 5)
    q[0], q[1] = LC.at_distance(bank[6], 0.2, rng), LC.at_distance(bank[6], 0.05, rng)
    F, lm = checked(records(q, rng), table(bank, rng))
    r1, r0 = RR.search(F, lm, mutual=True), RR.search(F, lm, mutual=False)
    assert list(r1["match"][:2]) == [-1, 6] and list(r0["match"][:2]) == [6, 6] and r1["n_pass"] == r0["n_pass"] == 2
    return F, lm


def reloc_scene(seed=7):
    """lmap_cases.chain_scene -- a noise-free frame at a known pose, about 200 candidate points that project exactly
    onto its keypoints with descriptors near theirs -- and a stale pose 3 m and 0.6 rad away from the truth
    -> (frame, table, ground truth T_wc, stale T_wc)"""
    from rspl_slam_amd import synthetic as SY
    fr, lm, gt, _ = LC.chain_scene(seed)
    stale = gt.copy()
    stale[:3, :3] = SY._rotvec_to_R(np.array([0.0, 0.6, 0.0])) @ gt[:3, :3]
    stale[:3, 3] += np.array([3.0, 0.0, 0.0])
    checked(fr["features"], lm)
    return dict(fr, Twc=stale), lm, gt, stale
