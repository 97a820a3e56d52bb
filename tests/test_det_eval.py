"""Detection mAP, CPU form (eda_amd/ap_helper.py): parity with goldens produced by running the reference's
models/ap_helper.py + utils/nms.py + utils/eval_det.py (tools/gen_golden_det_eval.py), scope checks, tie rules."""
import os
import types

import numpy as np
import pytest
import torch

import det_eval_fixtures as DF
from eda_amd import ap_helper as AH

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    z = np.load(os.path.join(GOLDEN, f"det_eval_{name}.npz"))
    ep = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("in_")}
    return z, ep


def cfg(name):
    return dict(DF.config(name), dataset_config=types.SimpleNamespace(num_class=DF.NUM_CLASS))


@pytest.mark.parametrize("name", list(DF.CASES))
def test_cpu_form_matches_reference(name):
    z, ep = load(name)
    c = cfg(name)
    preds = AH.parse_predictions(ep, c, DF.PREFIX, size_cls_agnostic=True)
    gts = AH.parse_groundtruths(ep, c, size_cls_agnostic=True)
    assert ep["batch_gt_map_cls"] is gts
    if c["cls_nms"]:
        pm = ep[f"{DF.PREFIX}pred_mask"]
        assert isinstance(pm, np.ndarray) and pm.dtype == np.float64
        np.testing.assert_array_equal(pm, z["pred_mask"])
    else:
        assert f"{DF.PREFIX}pred_mask" not in ep
    sc, cl, sv, co = DF.flatten(preds)
    np.testing.assert_array_equal(sc, z["pred_scene"])
    np.testing.assert_array_equal(cl, z["pred_cls"])
    np.testing.assert_allclose(sv, z["pred_score"], rtol=1e-6, atol=0)
    if "pred_corners" in z.files:
        np.testing.assert_array_equal(co, z["pred_corners"])
    assert all(isinstance(t[0], int) and t[1].shape == (8, 3) and t[1].dtype == np.float64 for p in preds for t in p)
    for t in DF.THRESHOLDS:
        tag = str(t).replace(".", "")
        calc = AH.APCalculator(t, None)
        calc.step(preds, gts)
        m = calc.compute_metrics()
        keys = [int(k.split()[0]) for k in m if k.endswith("Average Precision")]
        assert keys == list(z[f"classes_{tag}"])
        ap = np.array([m[f"{k} Average Precision"] for k in keys])
        rec = np.array([m[f"{k} Recall"] for k in keys])
        np.testing.assert_allclose(ap, z[f"ap_{tag}"], rtol=0, atol=1e-9)
        np.testing.assert_allclose(rec, z[f"rec_{tag}"], rtol=0, atol=1e-9)
        assert abs(m["mAP"] - float(z[f"map_{tag}"])) <= 1e-9
        assert abs(m["AR"] - float(z[f"ar_{tag}"])) <= 1e-9
        assert 0.1 < m["mAP"] < 0.9


def test_metric_keys_and_names():
    z, ep = load("eda")
    c = cfg("eda")
    names = {k: f"c{k}" for k in range(DF.NUM_CLASS)}
    calc = AH.APCalculator(0.25, names)
    calc.step(AH.parse_predictions(ep, c, DF.PREFIX, True), AH.parse_groundtruths(ep, c, True))
    m = calc.compute_metrics()
    keys = list(m)
    n = len(z["classes_025"])
    assert keys[:n] == [f"c{k} Average Precision" for k in z["classes_025"]]
    assert keys[n] == "mAP" and keys[-1] == "AR"
    assert keys[n + 1:-1] == [f"c{k} Recall" for k in z["classes_025"]]
    assert calc.uniq_gt_classes == set(int(k) for k in np.unique(ep["sem_cls_label"][ep["box_label_mask"] == 1]))


def test_records_on_cpu_equal_tuples():
    """CPU records (as_tensors=True) accumulated over several steps give the tuple path's metrics."""
    _, ep = load("eda")
    c = cfg("eda")
    tup = AH.APCalculator(0.25)
    tup.step(AH.parse_predictions(ep, c, DF.PREFIX, True), AH.parse_groundtruths(ep, c, True))
    recs = AH.APCalculator(0.25)
    for sl in (slice(0, 1), slice(1, 4)):
        sub = {k: v[sl] for k, v in ep.items()}
        p = AH.parse_predictions(sub, c, DF.PREFIX, True, as_tensors=True)
        assert isinstance(p, AH.DetPredictions) and p.aabb.dtype == torch.float64
        recs.step(p, AH.parse_groundtruths(sub, c, True, as_tensors=True))
    a, b = tup.compute_metrics(), recs.compute_metrics()
    assert list(a) == list(b)
    for k in a:
        assert abs(a[k] - b[k]) <= 1e-12, k
    with pytest.raises(TypeError):
        recs.step(AH.parse_predictions(ep, c, DF.PREFIX, True), AH.parse_groundtruths(ep, c, True))


@pytest.mark.parametrize("key,value,size_agnostic,match", [
    ("remove_empty_box", True, True, "remove_empty_box"),
    ("use_3d_nms", False, True, "2D NMS"),
    ("use_3d_nms", True, False, "size-class"),
])
def test_out_of_scope_options_raise(key, value, size_agnostic, match):
    _, ep = load("eda")
    c = cfg("eda")
    c[key] = value
    with pytest.raises(NotImplementedError, match=match):
        AH.parse_predictions(ep, c, DF.PREFIX, size_cls_agnostic=size_agnostic)
    if not size_agnostic:
        with pytest.raises(NotImplementedError, match="size-class"):
            AH.parse_groundtruths(ep, c, size_cls_agnostic=False)


def test_nms_ties_go_to_the_larger_index():
    box = np.array([0, 0, 0, 1, 1, 1], np.float64)
    aabb = np.stack([box, box, box + [5, 0, 0, 5, 0, 0], box])[None]        # 0, 1, 3 identical; 2 apart
    score = np.array([[0.5, 0.5, 0.5, 0.5]])
    cls = np.zeros((1, 4), np.int32)
    keep = AH.nms_3d(aabb, score, cls, 0.25, cls_nms=True)
    np.testing.assert_array_equal(keep, [[False, False, True, True]])
    # class gate: the same box of another class survives; old-type overlap divides by the later box's volume
    cls2 = np.array([[0, 1, 0, 0]], np.int32)
    np.testing.assert_array_equal(AH.nms_3d(aabb, score, cls2, 0.25, cls_nms=True), [[False, True, True, True]])
    np.testing.assert_array_equal(AH.nms_3d(aabb, score, cls2, 0.25, cls_nms=False), [[False, False, True, True]])
    small = np.array([[[0, 0, 0, 1, 1, 1], [0, 0, 0, 0.5, 1, 1]]], np.float64)
    sc2 = np.array([[0.9, 0.1]])
    assert AH.nms_3d(small, sc2, None, 0.6, old_type=True, cls_nms=False).tolist() == [[True, False]]
    assert AH.nms_3d(small, sc2, None, 0.6, old_type=False, cls_nms=False).tolist() == [[True, True]]


def test_zero_volume_boxes_never_suppress_each_other():
    flat = np.array([0, 0, 0, 1, 0, 1], np.float64)                          # zero height
    aabb = np.stack([flat, flat])[None]
    keep = AH.nms_3d(aabb, np.array([[0.9, 0.8]]), np.zeros((1, 2), np.int32), 0.25)
    assert keep.tolist() == [[True, True]]                                  # 0/0: NaN > thr is False


def test_ap_ties_in_insertion_order_and_first_maximum():
    """Equal confidences are taken in (scene, j) order; a prediction matches the FIRST of equally good boxes."""
    gt = np.array([0, 0, 0, 1, 1, 1], np.float64)
    calc = AH.APCalculator(0.5)
    corners = AH._corners_np(gt)
    far = AH._corners_np(gt + [9, 0, 0, 9, 0, 0])
    # scene 0: a miss then a hit at the same confidence -> insertion order puts the miss first
    calc.step([[(0, far, np.float32(0.5)), (0, corners, np.float32(0.5))]], [[(0, corners)]])
    m = calc.compute_metrics()
    # order FP, TP: precision [0, 0.5], recall [0, 1 / (1 + 1e-8)] -> AP = 0.5 / (1 + 1e-8)
    assert abs(m["0 Average Precision"] - 0.5 / (1 + 1e-8)) < 1e-12
    # two identical ground-truth boxes: both predictions pick the FIRST; the second finds it taken and is a false
    # positive (eval_det.py:228-235 does not fall back to the next-best box)
    calc.reset()
    calc.step([[(0, corners, np.float32(0.9)), (0, corners, np.float32(0.8))]], [[(0, corners), (0, corners)]])
    m = calc.compute_metrics()
    assert abs(m["0 Recall"] - 1 / (2 + 1e-8)) < 1e-12 and abs(m["0 Average Precision"] - 1 / (2 + 1e-8)) < 1e-12


def test_class_with_ground_truth_but_no_prediction_counts_zero():
    gt = AH._corners_np(np.array([0, 0, 0, 1, 1, 1], np.float64))
    calc = AH.APCalculator(0.25)
    calc.step([[(0, gt, np.float32(0.9))]], [[(0, gt), (3, gt)]])
    m = calc.compute_metrics()
    assert m["3 Average Precision"] == 0.0 and m["3 Recall"] == 0.0
    assert abs(m["mAP"] - 0.5 / (1 + 1e-8)) < 1e-12


def test_det_class_scores_sums_token_columns_in_order():
    torch.manual_seed(0)
    ep = {"proj_tokens": torch.randn(2, 30, 8), "last_proj_queries": torch.randn(2, 5, 8)}
    word, tok = [0, 0, 0, 1, 2, 2, 3], [1, 2, 3, 5, 7, 40, 200]             # token 200 lies in the zero padding
    out = AH.det_class_scores(ep, word, tok)
    s = torch.matmul(ep["last_proj_queries"], ep["proj_tokens"].transpose(-1, -2)) / 0.07
    pad = torch.zeros(2, 5, 256)
    pad[:, :, :30] = s
    ref = torch.zeros(2, 5, 4)
    for w, t in zip(word, tok):
        ref[..., w] += pad[..., t]
    assert torch.equal(out, ref) and ep["last_sem_cls_scores"] is out
