"""tests/golden/augment_<case>.npz: the REFERENCE's point-dependent dataset work (src/joint_det_dataset.py
Joint3DDataset._get_pc / _get_target_boxes / _get_scene_objects / _get_detected_objects with Scan from
src/visual_data_handlers.py; imported from /root/reference in this build container only) on synthetic scans.
    python tools/gen_golden_augment.py

The dataset and the scans are built with __new__ and hold only what those methods read.  h5py, wandb, sng_parser and
plyfile are not installed here and are stubbed.  np.random.rand / random / randint are wrapped to record every draw in
order; the golden stores the inputs, the draws, the reference's `augmentations` and the outputs cast as __getitem__
casts them.  Only arrays are stored.
"""
import importlib
import os
import sys
import tempfile
import types

import numpy as np

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
N_POINTS = 3000


def load_reference():
    for name in ("h5py", "wandb", "sng_parser", "plyfile"):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.PlyData = None
            sys.modules[name] = m
    sys.path.insert(0, REF)
    return importlib.import_module("src.joint_det_dataset")


class Recorder:
    """np.random.rand / random / randint, recording (name, value) of every call."""

    def __init__(self):
        self.log = []
        self._orig = {k: getattr(np.random, k) for k in ("rand", "random", "randint")}

    def __enter__(self):
        for k, f in self._orig.items():
            def wrap(*a, _f=f, _k=k, **kw):
                v = _f(*a, **kw)
                self.log.append((_k, np.asarray(v)))
                return v
            setattr(np.random, k, wrap)
        return self

    def __exit__(self, *exc):
        for k, f in self._orig.items():
            setattr(np.random, k, f)


def make_scan(J, rng, n_objects, replacement=False):
    """A Scan with N_POINTS points in a 6 x 5 x 3 m room and n_objects disjoint objects (labels cycle over valid and
    invalid class ids)."""
    Scan = sys.modules["src.visual_data_handlers"].Scan
    n_orig = N_POINTS // 2 if replacement else N_POINTS
    pc = rng.uniform([-3, -2.5, 0], [3, 2.5, 3], (n_orig, 3))
    # objects: contiguous runs of a random permutation (leaving ~10 % of the points in no object)
    perm = rng.permutation(n_orig)
    cuts = np.sort(rng.choice(np.arange(1, int(n_orig * 0.9)), n_objects - 1, replace=False))
    groups = np.split(perm[:int(n_orig * 0.9)], cuts)
    for g in groups:                      # compact objects: pull each object's points towards a centre
        c = rng.uniform([-2.5, -2, 0.2], [2.5, 2, 2.5])
        pc[g] = c + (pc[g] - pc[g].mean(0)) * rng.uniform(0.05, 0.3)
    color = (rng.randint(0, 256, (n_orig, 3)) / 256.0).astype(np.float32)
    if replacement:                       # Scan.load_point_cloud's keep-count sampling (visual_data_handlers.py:112-124)
        choices = rng.choice(n_orig, N_POINTS, replace=True)
        new_pts = np.zeros(n_orig).astype(int)
        new_pts[choices] = np.arange(len(choices)).astype(int)
        pc, color = pc[choices], color[choices]
        groups = [new_pts[g[np.isin(g, choices)]] for g in groups]
    scan = Scan.__new__(Scan)
    scan.orig_pc = pc.astype(np.float64)
    scan.pc = np.copy(scan.orig_pc)
    scan.color = color
    labels = [3, 4, 5, 6, 7, 0, 8, 9, 10, 2000]           # 0 and 2000 are no class: not kept
    scan.three_d_objects = [{"object_id": i, "points": np.array(g), "instance_label": f"l{labels[i % len(labels)]}"}
                            for i, g in enumerate(groups)]
    return scan


def make_dataset(J, split, data_path, butd=False, butd_cls=False, augment_det=False, detect_intermediate=False):
    ds = J.Joint3DDataset.__new__(J.Joint3DDataset)
    ds.split, ds.augment = split, split == "train"
    ds.use_color, ds.use_height, ds.use_multiview = True, False, False
    ds.mean_rgb = np.array([109.8, 97.2, 83.8]) / 256
    ds.butd, ds.butd_gt, ds.butd_cls, ds.augment_det = butd, False, butd_cls, augment_det
    ds.detect_intermediate = detect_intermediate
    ds.data_path = data_path
    ds.label_map = {f"l{i}": i for i in (0, 2, 3, 4, 5, 6, 7, 8, 9, 10, 2000)}
    return ds


CASES = {
    # name: (split, dataset, utterance, n_objects, target, flips wanted (yz, xz) or None, options)
    "rot_yz_butd_augdet": ("train", "scannet", "chair . table", 40, [1, 2, 3, 6], (True, False),
                           dict(butd=True, augment_det=True)),
    "rot_xz": ("train", "scannet", "chair . table", 30, [0, 4], (False, True), {}),
    "rot_both_butd": ("train", "scanrefer", "the chair near the table", 35, 7, (True, True), dict(butd=True)),
    "norotate_anchor": ("train", "nr3d", "the chair on the left of the table", 25, 3, None,
                        dict(detect_intermediate=True, anchor=11)),
    "eval_butd": ("val", "scanrefer", "the chair near the table", 30, 5, None, dict(butd=True)),
    "butd_cls": ("train", "scanrefer", "the chair near the table", 30, 2, None, dict(butd_cls=True)),
    "replacement": ("train", "scanrefer", "the big chair", 20, 4, None, {}),
    "many_objects": ("train", "scanrefer", "the small lamp", 150, 140, None, dict(butd=True)),
}


def run_case(J, name, seed):
    split, dataset, utt, n_obj, target, flips, opt = CASES[name]
    opt = dict(opt)
    anchor = opt.pop("anchor", None)
    rng = np.random.RandomState(seed)
    scan = make_scan(J, rng, n_obj, replacement=name == "replacement")
    anno = {"scan_id": f"scene{seed:04d}_00", "dataset": dataset, "utterance": utt, "target_id": target,
            "auxi_entity": {"lemma_head": "table"} if anchor is not None else None,
            "anchor_ids": [anchor] if anchor is not None else []}
    tmp = tempfile.mkdtemp()
    det_cls_names = None
    if opt.get("butd") or opt.get("butd_cls"):
        k = 20
        c = rng.uniform([-2.5, -2, 0.2], [2.5, 2, 2.5], (k, 3))
        s = rng.uniform(0.1, 1.5, (k, 3))
        det_cls_names = [f"l{v}" for v in rng.choice([3, 4, 5, 6, 7, 8, 9, 10], k)]
        d = os.path.join(tmp, "group_free_pred_bboxes", f"group_free_pred_bboxes_{split}")
        os.makedirs(d)
        np.save(os.path.join(d, anno["scan_id"] + ".npy"),
                {"box": np.concatenate([c - s / 2, c + s / 2], 1), "class": det_cls_names,
                 "logits": rng.randn(k, 485).astype(np.float32)}, allow_pickle=True)
    ds = make_dataset(J, split, tmp, **opt)
    np.random.seed(seed)
    with Recorder() as rec:
        scan.pc = np.copy(scan.orig_pc)
        point_cloud, augmentations, og_color = ds._get_pc(anno, scan)
        gt_bboxes, box_label_mask, point_instance_label = ds._get_target_boxes(anno, scan)
        class_ids, all_bboxes, all_bbox_label_mask = ds._get_scene_objects(scan)
        det_boxes, det_mask, det_cls, det_logits = ds._get_detected_objects(split, anno["scan_id"], augmentations)
    if flips is not None and (augmentations.get("yz_flip"), augmentations.get("xz_flip")) != flips:
        return None
    cls_results = None
    if opt.get("butd_cls"):                 # __getitem__: a perfect proposal stage with the classifier's class ids
        cls_results = np.arange(len(all_bboxes)) % 7
        det_boxes = all_bboxes
        det_cls = np.zeros(len(all_bboxes))
        det_cls[all_bbox_label_mask] = cls_results[all_bbox_label_mask]
    objs = [o["points"].astype(np.int64) for o in scan.three_d_objects]
    tids = target if isinstance(target, list) else [target] + ([anchor] if anchor is not None else [])
    out = dict(
        numpy_version=np.array(np.__version__), split=np.array(split), seed=np.array(seed),
        xyz=scan.orig_pc, color=scan.color, obj_points=np.concatenate(objs),
        obj_offsets=np.cumsum([0] + [len(o) for o in objs]), tids=np.array(tids, np.int64),
        keep=np.asarray(all_bbox_label_mask, bool),
        draw_names=np.array([k for k, _ in rec.log]),
        **{f"draw_{i}": v for i, (_, v) in enumerate(rec.log)},
        point_clouds=point_cloud.astype(np.float32), og_color=og_color.astype(np.float32),
        center_label=gt_bboxes[:, :3].astype(np.float32), size_gts=gt_bboxes[:, 3:].astype(np.float32),
        box_label_mask=box_label_mask.astype(np.float32), point_instance_label=point_instance_label.astype(np.int64),
        all_bboxes=all_bboxes.astype(np.float32), all_detected_boxes=det_boxes.astype(np.float32),
        all_detected_class_ids=det_cls.astype(np.int64), all_detected_logits_head=det_logits[:, :4].astype(np.float32),
    )
    for k in ("theta_z", "theta_x", "theta_y", "yz_flip", "xz_flip", "shift", "scale"):
        if k in augmentations:
            out["aug_" + k] = np.asarray(augmentations[k])
    if det_cls_names is not None and not opt.get("butd_cls"):
        raw = np.load(os.path.join(tmp, "group_free_pred_bboxes", f"group_free_pred_bboxes_{split}",
                                   anno["scan_id"] + ".npy"), allow_pickle=True).item()
        out["det_box_raw"] = np.asarray(raw["box"], np.float64)
        out["det_cls_raw"] = np.array([J.DC.nyu40id2class[ds.label_map[c]] for c in raw["class"]], np.int64)
    if cls_results is not None:
        out["butd_cls_ids"] = det_cls.astype(np.int64)
    return out


def main():
    J = load_reference()
    for i, name in enumerate(CASES):
        seed = 100 * (i + 1)
        while True:
            res = run_case(J, name, seed)
            if res is not None:
                break
            seed += 1
        path = os.path.join(OUT, f"augment_{name}.npz")
        np.savez_compressed(path, **res)
        print(path, os.path.getsize(path), "seed", seed)


if __name__ == "__main__":
    main()
