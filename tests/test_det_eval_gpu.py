"""Detection mAP on the MI355X (csrc/det_eval.hip through eda_amd/ap_helper.py): goldens of the reference, the explicit
NMS / matching entries against the CPU form at ScanNet-val size, accumulation, determinism, record vs tuple path."""
import os
import types

import numpy as np
import pytest
import torch

import det_eval_fixtures as DF
from eda_amd import ap_helper as AH

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = torch.device("cuda", 0)


def load(name):
    z = np.load(os.path.join(GOLDEN, f"det_eval_{name}.npz"))
    ep = {k[3:]: torch.from_numpy(z[k]).to(DEV) for k in z.files if k.startswith("in_")}
    return z, ep


def cfg(name):
    return dict(DF.config(name), dataset_config=types.SimpleNamespace(num_class=DF.NUM_CLASS))


def metrics_close(a, b, tol):
    assert list(a) == list(b)
    for k in a:
        assert abs(a[k] - b[k]) <= tol, (k, a[k], b[k])


@pytest.mark.parametrize("name", list(DF.CASES))
def test_gpu_matches_reference_goldens(name):
    z, ep = load(name)
    c = cfg(name)
    preds = AH.parse_predictions(ep, c, DF.PREFIX, size_cls_agnostic=True)
    gts = AH.parse_groundtruths(ep, c, size_cls_agnostic=True)
    if c["cls_nms"]:
        np.testing.assert_array_equal(ep[f"{DF.PREFIX}pred_mask"], z["pred_mask"])
    sc, cl, sv, co = DF.flatten(preds)
    np.testing.assert_array_equal(sc, z["pred_scene"])
    np.testing.assert_array_equal(cl, z["pred_cls"])
    np.testing.assert_allclose(sv, z["pred_score"], rtol=1e-5, atol=0)
    if "pred_corners" in z.files:
        np.testing.assert_array_equal(co, z["pred_corners"])
    # the device path: records accumulated on the GPU, both thresholds in one matching launch
    calc = AH.APCalculator(0.25)
    calc.step(AH.parse_predictions(ep, c, DF.PREFIX, True, as_tensors=True),
              AH.parse_groundtruths(ep, c, True, as_tensors=True))
    for t, m in zip(DF.THRESHOLDS, calc.compute_metrics_at(DF.THRESHOLDS)):
        tag = str(t).replace(".", "")
        keys = [int(k.split()[0]) for k in m if k.endswith("Average Precision")]
        assert keys == list(z[f"classes_{tag}"])
        np.testing.assert_allclose([m[f"{k} Average Precision"] for k in keys], z[f"ap_{tag}"], rtol=0, atol=1e-4)
        np.testing.assert_allclose([m[f"{k} Recall"] for k in keys], z[f"rec_{tag}"], rtol=0, atol=1e-4)
        assert abs(m["mAP"] - float(z[f"map_{tag}"])) <= 1e-4 and abs(m["AR"] - float(z[f"ar_{tag}"])) <= 1e-4


def _scannet_sized(seed=7, S=312, K=256, G=132):
    ep = DF.make_end_points(seed, S, K, G, objectness=False)
    aabb, obj, prob, sem = AH._decode_np(ep["last_center"], ep["last_pred_size"], ep["last_sem_cls_scores"], None)
    g_aabb = AH._aabb_np(ep["center_label"], ep["size_gts"])
    g_cls = np.where(ep["box_label_mask"] == 1, ep["sem_cls_label"], -1).astype(np.int32)
    return aabb, obj.astype(np.float64), prob, sem, g_aabb, g_cls


def test_explicit_entries_equal_cpu_form_at_scannet_val_size():
    aabb, score, prob, sem, g_aabb, g_cls = _scannet_sized()
    S, K, C = prob.shape
    keep_c = AH._nms_np(aabb, score, sem, 0.25, False, True)
    keep_g = AH.nms_3d(torch.from_numpy(aabb).to(DEV), torch.from_numpy(score).to(DEV), torch.from_numpy(sem).to(DEV),
                       0.25, old_type=False, cls_nms=True).cpu().numpy()
    np.testing.assert_array_equal(keep_g, keep_c)
    assert 0.1 < keep_c.mean() < 0.9
    conf = (prob * score.astype(np.float32)[..., None]).astype(np.float64)          # (S, K, C)
    valid = keep_c
    th = list(DF.THRESHOLDS)
    tp = AH.match_tp(*(torch.from_numpy(x).to(DEV) if x is not None else None
                       for x in (aabb, conf, None, valid, g_aabb, g_cls)), th, C)
    ap_g, rec_g, in_set = AH.ap_from_tp(tp, torch.from_numpy(conf).to(DEV), None, torch.from_numpy(valid).to(DEV),
                                        torch.from_numpy(g_cls).to(DEV), C)
    tp = tp.cpu().numpy()
    # the CPU form on the same flat predictions (scene, class-major, j)
    s_i, j_i = np.nonzero(valid)
    p_scene = np.repeat(s_i[None], C, 0).T.reshape(-1)
    p_j = np.repeat(j_i[None], C, 0).T.reshape(-1)
    p_cls = np.tile(np.arange(C), s_i.size)
    order = np.lexsort((p_j, p_cls, p_scene))
    p_scene, p_j, p_cls = p_scene[order], p_j[order], p_cls[order]
    gs, gj = np.nonzero(g_cls >= 0)
    matched = AH._match_np(p_scene, p_cls, aabb[p_scene, p_j], conf[p_scene, p_j, p_cls], gs, g_cls[gs, gj],
                           g_aabb[gs, gj], th)
    n_tp = 0
    for c, (idx, tpc) in matched.items():
        for t in range(len(th)):
            np.testing.assert_array_equal(tp[t, c, p_scene[idx], p_j[idx]], tpc[t])
            n_tp += int(tpc[t].sum())
    assert n_tp > 0 and int(tp.sum()) == n_tp                                    # and nothing else is flagged
    res = AH._metrics_np(p_scene, p_cls, aabb[p_scene, p_j], conf[p_scene, p_j, p_cls], gs, g_cls[gs, gj],
                         g_aabb[gs, gj], th)
    ap_g, rec_g = ap_g.cpu().numpy(), rec_g.cpu().numpy()
    assert in_set.all()
    for t, (ap, rec) in enumerate(res):
        for c in range(C):
            assert abs(ap_g[t, c] - ap[c]) <= 1e-12 and abs(rec_g[t, c] - rec[c]) <= 1e-12


def _records(ep, c, sl):
    sub = {k: v[sl] for k, v in ep.items()}
    return AH.parse_predictions(sub, c, DF.PREFIX, True, as_tensors=True), AH.parse_groundtruths(sub, c, True, True)


def test_several_steps_equal_one_step_and_runs_are_bit_identical():
    z, ep = load("eda")
    c = cfg("eda")
    one = AH.APCalculator(0.25)
    one.step(*_records(ep, c, slice(0, 4)))
    many = AH.APCalculator(0.25)
    for sl in (slice(0, 1), slice(1, 3), slice(3, 4)):
        many.step(*_records(ep, c, sl))
    a = one.compute_metrics_at(DF.THRESHOLDS)
    b = many.compute_metrics_at(DF.THRESHOLDS)
    assert a == b
    again = AH.APCalculator(0.25)
    again.step(*_records(ep, c, slice(0, 4)))
    assert again.compute_metrics_at(DF.THRESHOLDS) == a
    r1, r2 = _records(ep, c, slice(0, 4))[0], _records(ep, c, slice(0, 4))[0]
    for f in ("aabb", "keep", "valid", "conf", "sem_cls"):
        assert torch.equal(getattr(r1, f), getattr(r2, f)), f


@pytest.mark.parametrize("name", list(DF.CASES))
def test_device_records_equal_tuple_path(name):
    _, ep = load(name)
    c = cfg(name)
    tup = AH.APCalculator(0.5)
    tup.step(AH.parse_predictions(ep, c, DF.PREFIX, True), AH.parse_groundtruths(ep, c, True))
    rec = AH.APCalculator(0.5)
    rec.step(*_records(ep, c, slice(None)))
    metrics_close(tup.compute_metrics(), rec.compute_metrics(), 1e-12)


@pytest.mark.parametrize("K,G", [(100, 7), (1024, 1024)])
def test_proposal_counts(K, G):
    rng = np.random.default_rng(K)
    S, C = 3, 5
    lo = rng.uniform(-2, 2, (S, K, 3))
    aabb = np.concatenate([lo, lo + rng.uniform(0.05, 1.0, (S, K, 3))], -1)
    aabb[:, ::17] = aabb[:, ::17][:, :, [0, 1, 2, 3, 1, 5]]                    # zero-height boxes
    score = np.round(rng.uniform(0, 1, (S, K)), 3)                              # many exact ties
    cls = rng.integers(0, C, (S, K)).astype(np.int32)
    for cn, old in ((True, False), (False, True)):
        keep_c = AH._nms_np(aabb, score, cls, 0.25, old, cn)
        keep_g = AH.nms_3d(torch.from_numpy(aabb).to(DEV), torch.from_numpy(score).to(DEV),
                           torch.from_numpy(cls).to(DEV), 0.25, old_type=old, cls_nms=cn).cpu().numpy()
        np.testing.assert_array_equal(keep_g, keep_c)
    glo = rng.uniform(-2, 2, (S, G, 3))
    g_aabb = np.concatenate([glo, glo + rng.uniform(0.05, 1.0, (S, G, 3))], -1)
    g_cls = rng.integers(-1, C, (S, G)).astype(np.int32)
    conf = np.round(rng.uniform(0, 1, (S, K, 1)), 2)                            # ties in the AP order
    valid = keep_c
    tp = AH.match_tp(*(torch.from_numpy(x).to(DEV) for x in (aabb, conf, cls, valid, g_aabb, g_cls)), [0.1, 0.3], C)
    tp = tp.cpu().numpy()
    s_i, j_i = np.nonzero(valid)
    gs, gj = np.nonzero(g_cls >= 0)
    matched = AH._match_np(s_i, cls[s_i, j_i], aabb[s_i, j_i], conf[s_i, j_i, 0], gs, g_cls[gs, gj], g_aabb[gs, gj],
                           [0.1, 0.3])
    for c, (idx, tpc) in matched.items():
        for t in range(2):
            np.testing.assert_array_equal(tp[t, c, s_i[idx], j_i[idx]], tpc[t])


def test_scenes_without_ground_truth():
    _, ep = load("eda")
    c = cfg("eda")
    ep = dict(ep)
    ep["box_label_mask"] = torch.zeros_like(ep["box_label_mask"])
    calc = AH.APCalculator(0.25)
    calc.step(*_records(ep, c, slice(None)))
    m = calc.compute_metrics()
    aps = [v for k, v in m.items() if k.endswith("Average Precision")]
    assert len(aps) == DF.NUM_CLASS and all(v == 0.0 for v in aps) and m["mAP"] == 0.0 and m["AR"] == 0.0
    tup = AH.APCalculator(0.25)
    tup.step(AH.parse_predictions(ep, c, DF.PREFIX, True), AH.parse_groundtruths(ep, c, True))
    assert tup.compute_metrics() == m
