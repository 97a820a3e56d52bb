"""Cases of tests/golden/augment_*.npz (tools/gen_golden_augment.py: the reference's Joint3DDataset point work on
synthetic scans, every np.random draw recorded) turned into the inputs of eda_amd.augment."""
import glob
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(os.path.basename(p)[len("augment_"):-4] for p in glob.glob(os.path.join(GOLDEN, "augment_*.npz")))
KEYS = ("point_clouds", "og_color", "center_label", "size_gts", "box_label_mask", "point_instance_label",
        "all_bboxes", "all_detected_boxes", "all_detected_class_ids")


def load(name):
    z = np.load(os.path.join(GOLDEN, f"augment_{name}.npz"))
    return {k: z[k] for k in z.files}


def add_to_bank(bank, g):
    objs = np.split(g["obj_points"], g["obj_offsets"][1:-1])
    return bank.add_scan(g["xyz"], g["color"], objs, detected_boxes=g.get("det_box_raw"),
                         detected_class_ids=g.get("det_cls_raw"))


def inputs(g):
    """(params row, explicit draws, kwargs of augment_batch) of one golden case; the params row is built from the
    reference's own `augmentations` and recorded draws."""
    from eda_amd import augment as A
    train = str(g["split"]) == "train"
    names = list(g["draw_names"])
    draws = [g[f"draw_{i}"] for i in range(len(names))]
    n = len(g["xyz"])
    mode = "butd" if "det_box_raw" in g else ("butd_cls" if "butd_cls_ids" in g else "none")
    kw = dict(train=train, detected_mode=mode, targets=[g["tids"]], keep_mask=g["keep"][None],
              det_class_ids=g["butd_cls_ids"][None] if mode == "butd_cls" else None)
    if not train:
        return A.identity_params(1)[0], None, dict(kw, augment_det=False)
    big = [i for i, d in enumerate(draws) if d.shape == (n, 3)]
    i_noise, i_col = big
    rest = draws[i_col + 1:]
    augment_det = len(rest) == 5
    jt = 0.95 + 0.1 * rest[0]
    ja = 0.95 + 0.1 * rest[1]
    det = (rest[2], rest[3], rest[4]) if augment_det else (None, None, None)
    p = A.pack_draws(float(g["aug_theta_z"]), float(g["aug_theta_x"]), float(g["aug_theta_y"]),
                     bool(g.get("aug_yz_flip", False)), bool(g.get("aug_xz_flip", False)), g["aug_shift"],
                     float(g["aug_scale"]), jt, ja, *det)
    explicit = {"noise": (draws[i_noise] * 5e-3)[None], "color_factor": (0.98 + 0.04 * draws[i_col])[None]}
    return p, explicit, dict(kw, augment_det=augment_det)


def ulps_f32(a, b):
    """Elementwise distance in fp32 ulps (of the larger magnitude)."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    sp = np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64)
    return np.abs(a - b) / sp
