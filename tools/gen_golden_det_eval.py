"""tests/golden/det_eval_<case>.npz: the REFERENCE's detection evaluation (models/ap_helper.py parse_predictions /
parse_groundtruths / APCalculator, utils/nms.py, utils/eval_det.py, utils/box_util.py; imported from /root/reference in
this build container only) on the seeded end_points of tests/det_eval_fixtures.py.  Only arrays are stored.
    python tools/gen_golden_det_eval.py

A case is reseeded (seed + 1000, ...) when its outcome would rest on rounding rather than logic: two NMS scores of a
scene within 1e-5 (relative), an objectness within 1e-5 of conf_thresh, two confidences above 0.05 of one class within
1e-5, an IoU within 1e-9 of an AP threshold, or two different ground-truth IoUs of one prediction within 1e-9.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import det_eval_fixtures as DF  # noqa: E402
from eda_amd import ap_helper as AH  # noqa: E402  (only for the rounding checks below)


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    if "ipdb" not in sys.modules:
        stub = types.ModuleType("ipdb")
        stub.set_trace = lambda *a, **k: None
        sys.modules["ipdb"] = stub
    sys.path.insert(0, os.path.join(REF, "utils"))            # eval_det imports metric_util / box_util flat
    for pkg in ("models", "utils"):
        m = types.ModuleType(pkg)
        m.__path__ = []
        sys.modules[pkg] = m
    for name in ("box_util", "nms", "eval_det"):
        setattr(sys.modules["utils"], name, _load(f"utils.{name}", os.path.join(REF, "utils", f"{name}.py")))
    return _load("models.ap_helper", os.path.join(REF, "models", "ap_helper.py"))


def _torch(ep):
    return {k: torch.from_numpy(v.copy()) for k, v in ep.items()}


def _rounding_safe(ep, cfg, preds):
    obj_logits = ep.get(f"{DF.PREFIX}objectness_scores")
    aabb, obj, _, _ = AH._decode_np(ep[f"{DF.PREFIX}center"], ep[f"{DF.PREFIX}pred_size"],
                                    ep[f"{DF.PREFIX}sem_cls_scores"], obj_logits)
    for o in obj:
        s = np.sort(o.astype(np.float64))
        if np.any(np.diff(s) <= 1e-5 * np.abs(s[1:])):
            return "NMS scores"
        if np.any(np.abs(o.astype(np.float64) - cfg["conf_thresh"]) <= 1e-5):
            return "conf_thresh"
    sc, cl, sv, co = DF.flatten(preds)
    for c in np.unique(cl):
        s = np.sort(sv[(cl == c) & (sv > 0.05)])
        if np.any(np.diff(s) <= 1e-5 * s[1:]):
            return "confidences"
    g_aabb = AH._aabb_np(ep["center_label"], ep["size_gts"])
    p_aabb = np.concatenate([co.min(1), co.max(1)], -1)
    for i in range(len(sc)):
        b = sc[i]
        g = np.flatnonzero((ep["box_label_mask"][b] == 1) & (ep["sem_cls_label"][b] == cl[i]))
        if g.size == 0:
            continue
        iou = AH._iou_np(p_aabb[i][None], g_aabb[b, g])
        iou = iou[iou == iou]
        for t in DF.THRESHOLDS:
            if np.any(np.abs(iou - t) <= 1e-9):
                return "IoU at a threshold"
        u = np.sort(iou)
        d = np.diff(u)
        if np.any((d > 0) & (d <= 1e-9)):
            return "IoU near-tie"
    return None


def run_case(ref, name):
    cfg = DF.config(name)
    cfg_ref = dict(cfg, dataset_config=types.SimpleNamespace(num_class=DF.NUM_CLASS))
    seed = DF.CASES[name][0]
    while True:
        ep = DF.case_end_points(name, seed)
        ept = _torch(ep)
        preds = ref.parse_predictions(ept, cfg_ref, DF.PREFIX, size_cls_agnostic=True)
        why = _rounding_safe(ep, cfg, preds)
        if why is None:
            break
        print(name, "seed", seed, "reseeded:", why)
        seed += 1000
    gts = ref.parse_groundtruths(ept, cfg_ref, size_cls_agnostic=True)
    out = {f"in_{k}": v for k, v in ep.items()}
    out["seed"] = np.array(seed)
    if cfg["cls_nms"]:
        out["pred_mask"] = ept[f"{DF.PREFIX}pred_mask"].astype(np.float64)
    sc, cl, sv, co = DF.flatten(preds)
    out["pred_scene"], out["pred_cls"], out["pred_score"] = sc, cl, sv
    if name == "eda":
        out["pred_corners"] = co
    for t in DF.THRESHOLDS:
        calc = ref.APCalculator(t, None)
        calc.step(preds, gts)
        m = calc.compute_metrics()
        keys = sorted(int(k.split()[0]) for k in m if k.endswith("Average Precision"))
        tag = str(t).replace(".", "")
        out[f"classes_{tag}"] = np.array(keys, np.int64)
        out[f"ap_{tag}"] = np.array([m[f"{k} Average Precision"] for k in keys], np.float64)
        out[f"rec_{tag}"] = np.array([m[f"{k} Recall"] for k in keys], np.float64)
        out[f"map_{tag}"] = np.array(m["mAP"], np.float64)
        out[f"ar_{tag}"] = np.array(m["AR"], np.float64)
        print(name, t, "mAP %.4f AR %.4f" % (m["mAP"], m["AR"]), "predictions", len(sc),
              "kept", int(out["pred_mask"].sum()) if "pred_mask" in out else "-")
    return out


def main():
    ref = load_reference()
    for name in DF.CASES:
        out = run_case(ref, name)
        path = os.path.join(ROOT, "tests", "golden", f"det_eval_{name}.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
