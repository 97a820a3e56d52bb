"""Seeded synthetic end_points for the detection-mAP tests (eda_amd/ap_helper.py, tools/gen_golden_det_eval.py).

Proposals are jittered copies of ground-truth boxes plus clutter, so NMS suppresses a real fraction and the APs land
between about 0.1 and 0.9.  Every case also holds a scene without ground truth, exact duplicate proposals and
zero-volume (zero-height) proposals: their IoUs with each other are 0/0 = NaN."""
import numpy as np

PREFIX = "last_"
NUM_CLASS = 18
THRESHOLDS = (0.25, 0.5)

_BASE = {"remove_empty_box": False, "use_3d_nms": True, "nms_iou": 0.25, "use_old_type_nms": False, "cls_nms": True,
         "per_class_proposal": True, "conf_thresh": 0.0, "hungarian_loss": True}

# name -> (seed, B, K, G, objectness logits, config overrides); the first is EDA's evaluation configuration
CASES = {
    "eda": (101, 4, 100, 24, False, {}),
    "old_nocls": (202, 3, 130, 20, True, {"cls_nms": False, "use_old_type_nms": True, "per_class_proposal": False,
                                          "conf_thresh": 0.05}),
    "obj_cls_thresh": (303, 3, 64, 16, True, {"use_old_type_nms": True, "conf_thresh": 0.1}),
}


def config(name):
    cfg = dict(_BASE)
    cfg.update(CASES[name][5])
    return cfg


def make_end_points(seed, B, K, G, objectness, C=NUM_CLASS, empty_scene=1):
    """numpy end_points (float32 / int64), scene `empty_scene` without ground truth."""
    rng = np.random.default_rng(seed)
    center_label = np.zeros((B, G, 3), np.float32)
    size_gts = np.zeros((B, G, 3), np.float32)
    mask = np.zeros((B, G), np.float32)
    label = np.zeros((B, G), np.int64)
    center = np.zeros((B, K, 3), np.float32)
    size = np.zeros((B, K, 3), np.float32)
    logits = rng.normal(0.0, 1.0, (B, K, C + 1)).astype(np.float32)
    for b in range(B):
        n = 0 if b == empty_scene else int(rng.integers(G // 2, G + 1))
        center_label[b, :n] = rng.uniform([-3, -3, 0], [3, 3, 2], (n, 3))
        size_gts[b, :n] = rng.uniform(0.2, 1.5, (n, 3))
        mask[b, :n] = 1
        label[b, :n] = rng.integers(0, C, n)
        for k in range(K):
            if n and rng.random() < 0.65:
                g = int(rng.integers(0, n))
                s = size_gts[b, g]
                center[b, k] = center_label[b, g] + rng.normal(0, 0.15, 3) * s
                size[b, k] = s * np.clip(1 + rng.normal(0, 0.15, 3), 0.3, None)
                logits[b, k, label[b, g]] += rng.uniform(1.0, 4.0)
            else:
                center[b, k] = rng.uniform([-3, -3, 0], [3, 3, 2])
                size[b, k] = rng.uniform(0.1, 1.2, 3)
                logits[b, k, C] += rng.uniform(0.0, 3.0)
        # exact duplicates of earlier proposals (same box, other scores) and zero-volume boxes
        for k in rng.choice(np.arange(K // 2, K), 4, replace=False):
            src = int(rng.integers(0, K // 2))
            center[b, k], size[b, k] = center[b, src], size[b, src]
        for k in rng.choice(np.arange(0, K // 2), 3, replace=False):
            size[b, k, 2] = 0.0                       # zero height (a flat footprint keeps the reference's hull valid)
    ep = {f"{PREFIX}center": center, f"{PREFIX}pred_size": size, f"{PREFIX}sem_cls_scores": logits,
          "center_label": center_label, "size_gts": size_gts, "box_label_mask": mask, "sem_cls_label": label}
    if objectness:
        ep[f"{PREFIX}objectness_scores"] = rng.normal(0.5, 1.5, (B, K)).astype(np.float32)
    return ep


def case_end_points(name, seed=None):
    s, B, K, G, obj, _ = CASES[name]
    return make_end_points(s if seed is None else seed, B, K, G, obj)


def flatten(batch_pred_map_cls):
    """Tuple lists -> (scene, class, score, corners) arrays in list order."""
    sc, cl, sv, co = [], [], [], []
    for i, preds in enumerate(batch_pred_map_cls):
        for c, box, score in preds:
            sc.append(i)
            cl.append(int(c))
            sv.append(float(score))
            co.append(np.asarray(box, dtype=np.float64))
    return (np.asarray(sc, np.int64), np.asarray(cl, np.int64), np.asarray(sv, np.float64),
            np.asarray(co, np.float64).reshape(-1, 8, 3))
