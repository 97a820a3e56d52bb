"""Train-time scene augmentation and box targets (eda_amd/augment.py), CPU form: the reference's own outputs on the
golden cases (tools/gen_golden_augment.py), the host draws, the bank's checks and the Philox restatement."""
import numpy as np
import pytest
import torch

import augment_fixtures as F
from eda_amd import augment as A


@pytest.mark.parametrize("name", F.CASES)
def test_cpu_form_matches_reference(name):
    g = F.load(name)
    bank = A.SceneBank("cpu")
    slot = F.add_to_bank(bank, g)
    p, explicit, kw = F.inputs(g)
    out = A.augment_batch(bank, [slot], p[None], explicit=explicit, **kw)
    assert set(out) == set(F.KEYS)
    for k in F.KEYS:
        got, want = out[k].numpy()[0], g[k]
        assert got.shape == want.shape and got.dtype == want.dtype, (k, got.shape, got.dtype, want.shape, want.dtype)
        if want.dtype.kind == "f" and k != "box_label_mask":
            # the reference's np.matmul goes through BLAS, which may contract or order the sums differently
            assert F.ulps_f32(got, want).max() <= 1, k
        else:
            np.testing.assert_array_equal(got, want, err_msg=k)


def test_golden_cases_cover_the_issue():
    assert len(F.CASES) >= 8
    flips = set()
    for name in F.CASES:
        g = F.load(name)
        if "aug_yz_flip" in g:
            flips.add((bool(g["aug_yz_flip"]), bool(g["aug_xz_flip"])))
    assert {(True, False), (False, True), (True, True)} <= flips
    g = F.load("many_objects")
    assert len(g["obj_offsets"]) - 1 > 132 and g["tids"].max() >= 132
    g = F.load("replacement")
    covered = np.zeros(len(g["xyz"]), bool)
    covered[g["obj_points"]] = True
    # duplicates of the with-replacement sampling are in no object list
    assert len(np.unique(g["xyz"], axis=0)) < len(g["xyz"]) and not covered.all()


def test_draw_params_ranges():
    rng = np.random.RandomState(3)
    p = A.draw_params(rng, 400, rotate=True, augment_det=True)
    assert p.shape == (400, A.P_STRIDE) and p.dtype == np.float64
    tz = p[:, A.P_THETA]
    turns = np.round(tz / 90)
    assert set(np.unique(turns)) == {0, 1, 2, 3}
    assert np.abs(tz - 90 * turns).max() <= 5
    assert np.abs(p[:, A.P_THETA + 1:A.P_THETA + 3]).max() <= 2.5
    assert 0 < p[:, A.P_YZ].mean() < 1 and 0 < p[:, A.P_XZ].mean() < 1
    assert set(np.unique(p[:, [A.P_YZ, A.P_XZ]])) == {0.0, 1.0}
    sc = p[:, A.P_SCALE]
    assert sc.min() >= 0.98 and sc.max() < 1.02
    sh = p[:, A.P_SHIFT:A.P_SHIFT + 3]
    assert sh.min() >= -0.5 and sh.max() < 0.5
    for off in (A.P_JT, A.P_JA):
        j = p[:, off:off + 132 * 6]
        assert j.min() >= 0.95 and j.max() < 1.05
    assert p[:, A.P_RB:A.P_CR + 132].min() >= 0 and p[:, A.P_RB:A.P_CR + 132].max() < 1
    rc = p[:, A.P_RC:A.P_RC + 132]
    assert (rc == np.round(rc)).all() and rc.min() >= 0 and rc.max() < A.N_DET_CLASSES
    # rotation matrices are rot_z / rot_x / rot_y of the drawn angles
    for b in range(3):
        np.testing.assert_array_equal(p[b, A.P_RZ:A.P_RZ + 9], A.rot_z_matrix(p[b, A.P_THETA]).reshape(-1))
        np.testing.assert_array_equal(p[b, A.P_RY:A.P_RY + 9], A.rot_y_matrix(p[b, A.P_THETA + 2]).reshape(-1))
    # no rotation: no quarter turn, no flip
    q = A.draw_params(np.random.RandomState(4), 200, rotate=False)
    assert np.abs(q[:, A.P_THETA]).max() <= 5
    assert (q[:, [A.P_YZ, A.P_XZ]] == 0).all()
    assert (q[:, A.P_RB:] == 0).all()


def test_scene_bank_checks():
    bank = A.SceneBank("cpu")
    xyz = np.random.RandomState(0).rand(50, 3)
    col = np.zeros((50, 3), np.float32)
    with pytest.raises(ValueError, match="overlap"):
        bank.add_scan(xyz, col, [np.array([0, 1, 2]), np.array([2, 3])])
    with pytest.raises(ValueError, match="float64 or float32"):
        bank.add_scan(xyz.astype(np.int32), col, [])
    with pytest.raises(ValueError, match="color"):
        bank.add_scan(xyz, col.astype(np.float64), [])
    with pytest.raises(ValueError, match=r"\(N, 3\)"):
        bank.add_scan(xyz[:, :2], col[:, :2], [])
    with pytest.raises(ValueError, match="out of range"):
        bank.add_scan(xyz, col, [np.array([0, 50])])
    with pytest.raises(ValueError, match="1024"):
        bank.add_scan(xyz, col, [np.array([], np.int64)] * 1025)
    assert bank.add_scan(xyz, col, [np.array([0, 1]), np.array([5])]) == 0
    with pytest.raises(ValueError, match="50 points"):
        bank.add_scan(xyz[:40], col[:40], [])
    assert bank.add_scan(xyz.astype(np.float32), col, [np.array([3])]) == 1
    with pytest.raises(ValueError, match="target index"):
        A.augment_batch(bank, [1], A.identity_params(1), [[1]], train=False)
    with pytest.raises(NotImplementedError):
        A.augment_batch(bank, [0], A.identity_params(1), [[0]], use_height=True)
    with pytest.raises(NotImplementedError):
        A.augment_batch(bank, [0], A.identity_params(1), [[0]], use_multiview=True)


def test_growth_and_many_slots():
    rng = np.random.RandomState(1)
    bank = A.SceneBank("cpu", capacity=1)
    for i in range(5):
        xyz = rng.rand(64, 3)
        assert bank.add_scan(xyz, rng.rand(64, 3).astype(np.float32), [np.arange(i, i + 3)]) == i
    assert bank.n_slots == 5 and bank.xyz.shape[0] >= 5 and bank.generation >= 3
    out = A.augment_batch(bank, [4, 0], A.identity_params(2), [[0], [0]], train=False)
    np.testing.assert_array_equal(out["point_clouds"][0, :, :3].numpy(), bank.xyz[4].numpy().astype(np.float32))
    assert (out["point_instance_label"][0, 4:7] == 0).all() and (out["point_instance_label"][0, :4] == -1).all()
    assert (out["center_label"][:, 1:] == 1000).all()


def test_philox_known_answers():
    """Philox4x32-10 known-answer vectors of Random123 (kat_vectors)."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = A.philox4x32_10([np.array([c], np.uint32) for c in ctr], key)
        assert tuple(int(w[0]) for w in got) == want


def test_point_uniforms_rng_mode():
    u = A.point_uniforms(7, 11, 2, 5000)
    assert u.shape == (2, 5000, 6) and u.min() >= 0 and u.max() < 1
    assert abs(u.mean() - 0.5) < 0.01
    assert not np.array_equal(u, A.point_uniforms(7, 12, 2, 5000))
    assert not np.array_equal(u[0], u[1])
    np.testing.assert_array_equal(u, A.point_uniforms(7, 11, 2, 5000))
    # the CPU form in RNG mode uses exactly these draws
    rng = np.random.RandomState(2)
    bank = A.SceneBank("cpu")
    xyz = rng.rand(300, 3)
    col = rng.rand(300, 3).astype(np.float32)
    bank.add_scan(xyz, col, [np.arange(10)])
    p = A.draw_params(rng, 1)
    uu = A.point_uniforms(5, 9, 1, 300)
    a = A.augment_batch(bank, [0], p, [[0]], seed=5, counter=9)
    b = A.augment_batch(bank, [0], p, [[0]], explicit={"noise": uu[..., :3] * 5e-3, "color_factor": 0.98 + 0.04 * uu[..., 3:]})
    for k in F.KEYS:
        assert torch.equal(a[k], b[k]), k
