"""Train-time scene augmentation and box targets on the device: the point-dependent part of the reference's
`Joint3DDataset.__getitem__` (src/joint_det_dataset.py: `_augment` :421-466, `_get_target_boxes` :684-715,
`_get_scene_objects` :717-754, `_get_detected_objects` :785-855; `Scan._set_axis_align_bbox`,
src/visual_data_handlers.py:246-260) as two HIP launches per batch (csrc/augment.hip).

    SceneBank       the scans on the device: fp64 points, fp32 colours, a per-point object id, the detector's boxes
    draw_params     the host draws of a batch (numpy, the reference's distributions) packed into one fp64 array
    augment_batch   one batch -> the reference's keys (point_clouds, og_color, center_label, size_gts, box_label_mask,
                    point_instance_label, all_bboxes, all_detected_boxes, all_detected_class_ids)
    AugmentStage    static inputs / outputs and a device counter: capturable, replays draw new per-point values

The two per-point arrays (noise, colour factor) are drawn on the device with Philox4x32-10 keyed by the seed; the
counter is (point, scene position << 2 | call, device counter lo, hi), call j giving the doubles of components 2j and
2j + 1 of (noise x, y, z, colour r, g, b).  Everything else is drawn on the host.  CPU tensors take a numpy form with the
same arithmetic and the same Philox restatement (`cpu_form`); the GPU tests compare the kernels with it bit for bit.

Class ids, label masks, text maps, tokens and the auxi_box decision stay on the host (INTEGRATION.md shows the
dataset override).  `use_height` and `use_multiview` are not supported.
"""
import ctypes

import numpy as np
import torch

from . import _lib

MAX_NUM_OBJ = 132
MAX_OBJECTS = 1024
MEAN_RGB = np.array([109.8, 97.2, 83.8]) / 256
N_DET_CLASSES = 485              # len(DC.nyu40ids) of the reference's 485-class ScannetDatasetConfig

# row layouts of csrc/augment.hip (checked against eda_augment_layout on first use)
ROWS = MAX_NUM_OBJ
I_SLOT, I_NT, I_TIDS = 0, 1, 4
I_KEEP = I_TIDS + ROWS
I_DCLS = I_KEEP + ROWS
I_STRIDE = I_DCLS + ROWS
P_RZ, P_RX, P_RY, P_YZ, P_XZ, P_SHIFT, P_SCALE, P_THETA, P_JT = 0, 9, 18, 27, 28, 29, 32, 33, 36
P_JA = P_JT + ROWS * 6
P_RB = P_JA + ROWS * 6
P_CR = P_RB + ROWS * 6
P_RC = P_CR + ROWS
P_STRIDE = P_RC + ROWS

DET_MODES = {"none": 0, "butd": 1, "butd_gt": 2, "butd_cls": 2}
OUT_KEYS = ("point_clouds", "og_color", "center_label", "size_gts", "box_label_mask", "point_instance_label",
            "all_bboxes", "all_detected_boxes", "all_detected_class_ids")
IN_KEYS = ("augment_ints", "augment_params")

_layout_checked = False


def _check_layout():
    global _layout_checked
    if not _layout_checked:
        out = (ctypes.c_int * 6)()
        _lib.check(_lib.lib().eda_augment_layout(out), "eda_augment_layout")
        want = (I_STRIDE, P_STRIDE, ROWS, MAX_OBJECTS, I_TIDS, P_JT)
        if tuple(out) != want:
            raise _lib.EdaHipError(f"augment row layout {tuple(out)} != {want}")
        _layout_checked = True


# ------------------------------------------------------------------------------------------------ rotations (host)
def rot_x_matrix(theta):
    """The matrix of the reference's rot_x (src/joint_det_dataset.py:1180-1190)."""
    theta = theta * np.pi / 180
    return np.array([[1.0, 0, 0], [0, np.cos(theta), -np.sin(theta)], [0, np.sin(theta), np.cos(theta)]])


def rot_y_matrix(theta):
    theta = theta * np.pi / 180
    return np.array([[np.cos(theta), 0, np.sin(theta)], [0, 1.0, 0], [-np.sin(theta), 0, np.cos(theta)]])


def rot_z_matrix(theta):
    theta = theta * np.pi / 180
    return np.array([[np.cos(theta), -np.sin(theta), 0], [np.sin(theta), np.cos(theta), 0], [0, 0, 1.0]])


def pack_draws(theta_z, theta_x, theta_y, yz_flip, xz_flip, shift, scale, target_jitter=None, all_jitter=None,
               det_rand_box=None, det_corrupt=None, det_rand_cls=None):
    """One scene's host draws -> its fp64 params row.  Jitters are the factors (0.95 + 0.1 * u), (n <= 132, 6); the
    augment_det arrays are the raw draws (random((132, 6)), random(132), randint(0, C, 132)).  Missing rows: 1 / 0."""
    p = np.zeros(P_STRIDE)
    p[P_RZ:P_RZ + 9] = rot_z_matrix(theta_z).reshape(-1)
    p[P_RX:P_RX + 9] = rot_x_matrix(theta_x).reshape(-1)
    p[P_RY:P_RY + 9] = rot_y_matrix(theta_y).reshape(-1)
    p[P_YZ], p[P_XZ] = float(bool(yz_flip)), float(bool(xz_flip))
    p[P_SHIFT:P_SHIFT + 3] = np.asarray(shift, np.float64).reshape(3)
    p[P_SCALE] = scale
    p[P_THETA:P_THETA + 3] = (theta_z, theta_x, theta_y)
    for off, arr in ((P_JT, target_jitter), (P_JA, all_jitter)):
        blk = np.ones((ROWS, 6))
        if arr is not None:
            arr = np.asarray(arr, np.float64).reshape(-1, 6)
            blk[:len(arr)] = arr
        p[off:off + ROWS * 6] = blk.reshape(-1)
    if det_rand_box is not None:
        p[P_RB:P_RB + ROWS * 6] = np.asarray(det_rand_box, np.float64).reshape(-1)
        p[P_CR:P_CR + ROWS] = np.asarray(det_corrupt, np.float64).reshape(-1)
        p[P_RC:P_RC + ROWS] = np.asarray(det_rand_cls, np.float64).reshape(-1)
    return p


def identity_params(batch):
    """Params of non-train batches (augment=False): identity rotations, no flip, shift 0, scale 1, unit jitters."""
    return np.stack([pack_draws(0.0, 0.0, 0.0, False, False, np.zeros(3), 1.0) for _ in range(batch)])


def draw_params(rng, batch, *, rotate=True, augment_det=False, n_det_classes=N_DET_CLASSES):
    """The host draws of a training batch with the reference's distributions, in its order per scene (_augment's angles,
    flips, shift and scale; the 132 x 6 target and scene-object jitters; augment_det's boxes, corruption draws and class
    ids).  rng: np.random.RandomState (or the np.random module).  rotate: bool or one per scene (False: no 90-degree
    turn and no flips, as for view-dependent utterances).  Returns (batch, P_STRIDE) fp64."""
    rot = np.broadcast_to(np.asarray(rotate, bool), (batch,))
    rows = []
    for b in range(batch):
        if rot[b]:
            theta_z = 90 * rng.randint(0, 4) + (2 * rng.random_sample() - 1) * 5
            yz = rng.random_sample() > 0.5
            xz = rng.random_sample() > 0.5
        else:
            theta_z = (2 * rng.random_sample() - 1) * 5
            yz = xz = False
        theta_x = (2 * rng.random_sample() - 1) * 2.5
        theta_y = (2 * rng.random_sample() - 1) * 2.5
        shift = rng.random_sample((3,))[None, :] - 0.5
        scale = 0.98 + 0.04 * rng.random_sample()
        jt = 0.95 + 0.1 * rng.random_sample((ROWS, 6))
        ja = 0.95 + 0.1 * rng.random_sample((ROWS, 6))
        det = (None, None, None)
        if augment_det:
            det = (rng.random_sample((ROWS, 6)), rng.random_sample(ROWS), rng.randint(0, n_det_classes, ROWS))
        rows.append(pack_draws(theta_z, theta_x, theta_y, yz, xz, shift, scale, jt, ja, *det))
    return np.stack(rows)


# -------------------------------------------------------------------------------------------------------- the bank
class SceneBank:
    """The scans of a dataset on one device (or on the CPU, for the numpy form).  Every scan has the same number of
    points (the reference's keep count).  Per slot: xyz fp64, colour fp32, a per-point object id (int16, -1 = in no
    object), the detector's boxes as centre / size fp64 (132 rows, zero padded) with their class ids and logits.

    Storage grows by doubling; a capture keeps references to the tensors it read, so a grown bank never frees memory a
    graph still reads (AugmentStage.check() tells when a stage is stale)."""

    def __init__(self, device, capacity=16):
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.n_points = None
        self.n_slots = 0
        self.max_objects = 1
        self.generation = 0
        self._cap = max(1, int(capacity))
        self.xyz = self.color = self.obj = self.det_box = self.det_cls = self.det_logits = None
        self._n_objects = []
        self._raw_boxes = []

    def _grow(self, need, n_logit_cols):
        N = self.n_points
        if self.xyz is not None and need <= self.xyz.shape[0]:
            return
        cap = self._cap if self.xyz is None else max(need, 2 * self.xyz.shape[0])
        dev = self.device
        new = dict(xyz=torch.zeros(cap, N, 3, dtype=torch.float64, device=dev),
                   color=torch.zeros(cap, N, 3, dtype=torch.float32, device=dev),
                   obj=torch.full((cap, N), -1, dtype=torch.int16, device=dev),
                   det_box=torch.zeros(cap, ROWS, 6, dtype=torch.float64, device=dev),
                   det_cls=torch.zeros(cap, ROWS, dtype=torch.int32, device=dev),
                   det_logits=torch.zeros(cap, ROWS, n_logit_cols, dtype=torch.float32, device=dev))
        for k, t in new.items():
            old = getattr(self, k)
            if old is not None:
                t[:self.n_slots].copy_(old[:self.n_slots])
            setattr(self, k, t)
        self.generation += 1

    def add_scan(self, xyz, color, object_points, detected_boxes=None, detected_class_ids=None, detected_logits=None):
        """xyz (N, 3) fp64 or fp32 (Scan.pc after align_to_axes), color (N, 3) fp32 (Scan.color), object_points: one
        index array per object in the scan's order (three_d_objects[i]['points']; disjoint, at most 1024 objects).
        detected_boxes (K, 6) as the detector file stores them (x1, y1, z1, x2, y2, z2), K < 132, with class ids (K,)
        (already mapped to class indices) and logits (K, C).  Returns the slot."""
        xyz = np.asarray(xyz)
        color = np.asarray(color)
        if xyz.ndim != 2 or xyz.shape[1] != 3 or xyz.dtype not in (np.float64, np.float32):
            raise ValueError(f"xyz must be (N, 3) float64 or float32, got {xyz.shape} {xyz.dtype}")
        if color.shape != xyz.shape or color.dtype != np.float32:
            raise ValueError(f"color must be (N, 3) float32 like xyz, got {color.shape} {color.dtype}")
        N = len(xyz)
        if N < 1:
            raise ValueError("a scan needs at least one point")
        if self.n_points is None:
            self.n_points = N
        elif N != self.n_points:
            raise ValueError(f"every scan of a bank has {self.n_points} points, got {N}")
        if len(object_points) > MAX_OBJECTS:
            raise ValueError(f"at most {MAX_OBJECTS} objects per scan, got {len(object_points)}")
        obj = np.full(N, -1, np.int16)
        count = np.zeros(N, np.int64)
        for i, pts in enumerate(object_points):
            pts = np.asarray(pts)
            if pts.size and (pts.dtype.kind not in "iu" or pts.ndim != 1):
                raise ValueError(f"object {i}: point indices must be a 1-D integer array")
            pts = pts.astype(np.int64)
            if pts.size and (pts.min() < 0 or pts.max() >= N):
                raise ValueError(f"object {i}: point index out of range")
            np.add.at(count, pts, 1)
            obj[pts] = i
        if (count > 1).any():
            raise ValueError("object point lists overlap (a point belongs to more than one object)")
        xyz64 = xyz.astype(np.float64)
        dbox = np.zeros((ROWS, 6))
        dcls = np.zeros(ROWS, np.int32)
        logits = None
        if detected_boxes is not None:
            box = np.asarray(detected_boxes, np.float64).reshape(-1, 6)
            if len(box) >= ROWS:
                raise ValueError(f"at most {ROWS - 1} detected boxes per scan (the reference asserts it)")
            dbox[:len(box)] = np.concatenate(((box[:, :3] + box[:, 3:]) * 0.5, box[:, 3:] - box[:, :3]), 1)
            if detected_class_ids is not None:
                cid = np.asarray(detected_class_ids).reshape(-1)
                if len(cid) != len(box):
                    raise ValueError("one class id per detected box")
                dcls[:len(cid)] = cid
            if detected_logits is not None:
                logits = np.asarray(detected_logits, np.float32).reshape(len(box), -1)
        n_logit_cols = N_DET_CLASSES if self.det_logits is None else self.det_logits.shape[-1]
        if logits is not None and logits.shape[1] != n_logit_cols:
            raise ValueError(f"detected_logits must have {n_logit_cols} columns")
        slot = self.n_slots
        self._grow(slot + 1, n_logit_cols)
        self.xyz[slot].copy_(torch.from_numpy(xyz64))
        self.color[slot].copy_(torch.from_numpy(np.ascontiguousarray(color)))
        self.obj[slot].copy_(torch.from_numpy(obj))
        self.det_box[slot].copy_(torch.from_numpy(dbox))
        self.det_cls[slot].copy_(torch.from_numpy(dcls))
        if logits is not None:
            self.det_logits[slot, :len(logits)].copy_(torch.from_numpy(logits))
        self.n_slots += 1
        self._n_objects.append(len(object_points))
        self.max_objects = max(self.max_objects, len(object_points))
        self._raw_boxes.append(np.stack([_box_cs(*_minmax(xyz64[np.asarray(p, np.int64)])) for p in object_points])
                               if object_points else np.zeros((0, 6)))
        return slot

    def n_objects(self, slot):
        return self._n_objects[slot]

    def object_boxes(self, slot):
        """(n_objects, 6) fp64 centre / size boxes of the scan's raw points (no augmentation, no jitter): what the host
        decides the auxi_box question from."""
        return self._raw_boxes[slot]

    def detected_logits(self, slots):
        """all_detected_logits of a batch (B, 132, C) fp32 (augmentation does not touch them)."""
        return self.det_logits.index_select(0, torch.as_tensor(slots, dtype=torch.int64, device=self.device))


def _minmax(p):
    if len(p) == 0:
        return np.zeros(3), np.zeros(3), True
    return p.min(0), p.max(0), False


def _box_cs(mn, mx, empty=False):
    """Scan._set_axis_align_bbox + the (min + max) * 0.5 / max - min conversion, fp64; an empty object: zeros."""
    if empty:
        return np.zeros(6)
    cx = (mx + mn) / 2.0
    lx = mx - mn
    lo = cx - lx / 2.0
    hi = cx + lx / 2.0
    return np.concatenate(((lo + hi) * 0.5, hi - lo))


# ---------------------------------------------------------------------------------------------------- packing
def pack_targets(bank, slots, targets, keep_mask=None, det_class_ids=None):
    """Per scene the int32 row of the kernels: slot, number of targets, target object ids (tids, < 132 of them, any
    object index), the scene-object keep mask (132; cleared beyond the scan's objects) and, for butd_gt / butd_cls,
    the detected class ids."""
    slots = np.asarray(slots, np.int64).reshape(-1)
    B = len(slots)
    if len(targets) != B:
        raise ValueError("one target list per scene")
    ints = np.zeros((B, I_STRIDE), np.int32)
    keep = np.zeros((B, ROWS), bool) if keep_mask is None else np.asarray(keep_mask, bool).reshape(B, ROWS)
    for b, s in enumerate(slots):
        if s < 0 or s >= bank.n_slots:
            raise ValueError(f"slot {s} is not in the bank ({bank.n_slots} scans)")
        tids = np.asarray(targets[b], np.int64).reshape(-1)
        if len(tids) > ROWS:
            raise ValueError(f"at most {ROWS} targets per scene")
        nobj = bank.n_objects(int(s))
        if len(tids) and (tids.min() < 0 or tids.max() >= nobj):
            raise ValueError(f"scene {b}: target index out of range (the scan has {nobj} objects)")
        ints[b, I_SLOT] = s
        ints[b, I_NT] = len(tids)
        ints[b, I_TIDS:I_TIDS + ROWS] = -1
        ints[b, I_TIDS:I_TIDS + len(tids)] = tids
        ints[b, I_KEEP:I_KEEP + ROWS] = keep[b] & (np.arange(ROWS) < nobj)
        if det_class_ids is not None:
            ints[b, I_DCLS:I_DCLS + ROWS] = np.asarray(det_class_ids[b]).reshape(ROWS)
    return ints


def empty_outputs(batch, n_points, device, use_color=True):
    dev = torch.device(device)
    f32 = dict(dtype=torch.float32, device=dev)
    return {
        "point_clouds": torch.empty(batch, n_points, 6 if use_color else 3, **f32),
        "og_color": torch.empty(batch, n_points, 3, **f32),
        "center_label": torch.empty(batch, ROWS, 3, **f32),
        "size_gts": torch.empty(batch, ROWS, 3, **f32),
        "box_label_mask": torch.empty(batch, ROWS, **f32),
        "point_instance_label": torch.empty(batch, n_points, dtype=torch.int64, device=dev),
        "all_bboxes": torch.empty(batch, ROWS, 6, **f32),
        "all_detected_boxes": torch.empty(batch, ROWS, 6, **f32),
        "all_detected_class_ids": torch.empty(batch, ROWS, dtype=torch.int64, device=dev),
    }


def _workspace(batch, n_obj, device):
    ws = torch.empty(batch * n_obj, 2, 3, dtype=torch.int64, device=device)
    ws[:, 0].fill_(-1)          # min keys: all ones
    ws[:, 1].fill_(0)           # max keys: zero
    return ws


def _check_out(out, batch, n_points, device, use_color):
    want = empty_outputs(batch, n_points, "meta", use_color)
    for k in OUT_KEYS:
        t = out[k]
        if t.shape != want[k].shape or t.dtype != want[k].dtype or not t.is_contiguous() or t.device != device:
            raise ValueError(f"out[{k!r}] must be a contiguous {tuple(want[k].shape)} {want[k].dtype} tensor on {device}")


def _launch(bank, ints, params, B, n_obj, train, use_color, det_mode, augment_det, noise, colf, counter_ptr,
            counter_value, seed, ws, out, stream):
    _check_layout()
    p = lambda t: t.data_ptr() if t is not None else None        # noqa: E731
    rc = _lib.lib().eda_augment_batch_f64(
        p(bank.xyz), p(bank.color), p(bank.obj), p(bank.det_box), p(bank.det_cls), bank.xyz.shape[0], bank.n_points,
        n_obj, p(ints), p(params), B, int(train), int(use_color), det_mode, int(augment_det), p(noise), p(colf),
        counter_ptr, int(counter_value), int(seed) & 0xFFFFFFFFFFFFFFFF, p(ws),
        *[p(out[k]) for k in ("point_clouds", "og_color", "point_instance_label", "center_label", "size_gts",
                              "box_label_mask", "all_bboxes", "all_detected_boxes", "all_detected_class_ids")],
        stream)
    _lib.check(rc, "eda_augment_batch_f64")


def augment_batch(bank, slots, params, targets, keep_mask=None, detected_mode="none", *, augment_det=False, train=True,
                  use_color=True, det_class_ids=None, seed=0, counter=0, explicit=None, out=None, use_height=False,
                  use_multiview=False):
    """Augment a batch of scans of `bank` and build its box targets.  slots (B,), params (B, P_STRIDE) from draw_params
    (train) or identity_params, targets: per scene the target object ids (tids, in order), keep_mask (B, 132) bool: the
    scene objects kept in all_bboxes (the class-validity mask of _get_scene_objects), detected_mode: "none", "butd"
    (the detector's boxes, + augment_det), "butd_gt" / "butd_cls" (a copy of all_bboxes, with det_class_ids (B, 132)).
    explicit: {"noise": (B, N, 3), "color_factor": (B, N, 3)} fp64 per-point draws (noise = u * 5e-3, factor = 0.98 +
    0.04 * u) instead of the Philox draws keyed by (seed, counter).  train=False: no augmentation, no jitter.
    Returns (or fills `out`) the reference's keys with __getitem__'s shapes and dtypes."""
    if use_height or use_multiview:
        raise NotImplementedError("use_height / use_multiview are not supported by the device augmentation")
    if detected_mode not in DET_MODES:
        raise ValueError(f"detected_mode must be one of {sorted(DET_MODES)}")
    det_mode = DET_MODES[detected_mode]
    if det_mode == 2 and det_class_ids is None:
        raise ValueError(f"detected_mode {detected_mode!r} needs det_class_ids")
    slots = np.asarray(slots, np.int64).reshape(-1)
    B, N = len(slots), bank.n_points
    params = np.asarray(params, np.float64)
    if params.shape != (B, P_STRIDE):
        raise ValueError(f"params must be ({B}, {P_STRIDE}) float64")
    ints = pack_targets(bank, slots, targets, keep_mask, det_class_ids)
    if bank.device.type == "cpu":
        res = cpu_form(bank, ints, params, train=train, use_color=use_color, det_mode=det_mode, augment_det=augment_det,
                       seed=seed, counter=counter, explicit=explicit)
        if out is None:
            return {k: torch.from_numpy(v) for k, v in res.items()}
        for k in OUT_KEYS:
            out[k].copy_(torch.from_numpy(res[k]))
        return out
    dev = bank.device
    if out is None:
        out = empty_outputs(B, N, dev, use_color)
    _check_out(out, B, N, dev, use_color)
    noise = colf = None
    if explicit is not None and train:
        noise = torch.as_tensor(np.asarray(explicit["noise"], np.float64).reshape(B, N, 3), device=dev).contiguous()
        colf = torch.as_tensor(np.asarray(explicit["color_factor"], np.float64).reshape(B, N, 3), device=dev).contiguous()
    ints_d = torch.from_numpy(ints).to(dev)
    params_d = torch.from_numpy(params).to(dev)
    ws = _workspace(B, bank.max_objects, dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    _launch(bank, ints_d, params_d, B, bank.max_objects, train, use_color, det_mode, augment_det, noise, colf, None,
            counter, seed, ws, out, stream)
    return out


# ------------------------------------------------------------------------------------------- the captured stage
class AugmentStage:
    """The augmentation of one batch shape as a capturable callable: static input buffers (`ints`, `params`; fill them
    with `set_inputs` or hand them over as the batch keys `augment_ints` / `augment_params`), static outputs (`out`,
    the keys in `produces`), and a device counter that every run reads and then bumps -- a replayed graph draws new
    per-point values each time, and get_counter / set_counter make the stream checkpointable."""

    produces = ("point_clouds", "og_color", "center_label", "size_gts", "box_label_mask", "point_instance_label",
                "all_bboxes", "all_detected_boxes", "all_detected_class_ids")
    consumes = IN_KEYS

    def __init__(self, bank, batch, *, train=True, use_color=True, detected_mode="none", augment_det=False, seed=0,
                 counter=0):
        if bank.device.type != "cuda":
            raise ValueError("AugmentStage runs on the GPU (augment_batch has the CPU form)")
        if detected_mode not in DET_MODES:
            raise ValueError(f"detected_mode must be one of {sorted(DET_MODES)}")
        self.bank, self.batch = bank, int(batch)
        self.train, self.use_color = bool(train), bool(use_color)
        self.detected_mode, self.det_mode, self.augment_det = detected_mode, DET_MODES[detected_mode], bool(augment_det)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        dev = bank.device
        self.n_obj = bank.max_objects
        self._bank_tensors = (bank.xyz, bank.color, bank.obj, bank.det_box, bank.det_cls)   # kept alive for the graph
        self._n_slots = bank.xyz.shape[0]
        self._generation = bank.generation
        self.ints = torch.zeros(self.batch, I_STRIDE, dtype=torch.int32, device=dev)
        self.params = torch.from_numpy(identity_params(self.batch)).to(dev)
        self.out = empty_outputs(self.batch, bank.n_points, dev, use_color)
        self.counter = torch.full((1,), int(counter), dtype=torch.int64, device=dev)
        self.ws = _workspace(self.batch, self.n_obj, dev)

    def pack(self, slots, params, targets, keep_mask=None, det_class_ids=None):
        """The stage's inputs of one batch as host tensors {augment_ints, augment_params} (a loader's next_batch keys)."""
        self.check()
        params = np.asarray(params, np.float64)
        if params.shape != (self.batch, P_STRIDE):
            raise ValueError(f"params must be ({self.batch}, {P_STRIDE}) float64")
        if self.det_mode == 2 and det_class_ids is None:
            raise ValueError(f"detected_mode {self.detected_mode!r} needs det_class_ids")
        ints = pack_targets(self.bank, slots, targets, keep_mask, det_class_ids)
        if (ints[:, I_SLOT] >= self._n_slots).any():
            raise ValueError("a slot was added to the bank after this stage was built")
        return {"augment_ints": torch.from_numpy(ints), "augment_params": torch.from_numpy(params.copy())}

    def set_inputs(self, slots, params, targets, keep_mask=None, det_class_ids=None):
        """Copy one batch's inputs into the static buffers (on the current stream)."""
        p = self.pack(slots, params, targets, keep_mask, det_class_ids)
        self.ints.copy_(p["augment_ints"])
        self.params.copy_(p["augment_params"])

    def bind(self, inputs=None, outputs=None):
        """Use other (contiguous, same shape and dtype) tensors as the static inputs / outputs, e.g. a pipeline's batch
        buffers.  Call before capturing."""
        for k, t in (inputs or {}).items():
            name = {"augment_ints": "ints", "augment_params": "params"}[k]
            cur = getattr(self, name)
            if t.shape != cur.shape or t.dtype != cur.dtype or not t.is_contiguous():
                raise ValueError(f"{k}: needs a contiguous {tuple(cur.shape)} {cur.dtype} tensor")
            setattr(self, name, t)
        if outputs:
            out = dict(self.out)
            out.update(outputs)
            _check_out(out, self.batch, self.bank.n_points, self.bank.device, self.use_color)
            self.out = out

    def check(self):
        """Raises when the bank has grown past what this stage was built for (its graph would not see the new scans)."""
        if self.bank.max_objects > self.n_obj or self.bank.generation != self._generation:
            raise RuntimeError("the SceneBank grew after this AugmentStage was built: build a new stage")

    def __call__(self):
        """Launch the augmentation of the batch in the static inputs (capturable); the counter advances by one."""
        self.check()
        stream = torch.cuda.current_stream(self.bank.device).cuda_stream
        _launch(self.bank, self.ints, self.params, self.batch, self.n_obj, self.train, self.use_color, self.det_mode,
                self.augment_det, None, None, self.counter.data_ptr(), 0, self.seed, self.ws, self.out, stream)
        return self.out

    run = __call__

    def get_counter(self):
        return int(self.counter.item())

    def set_counter(self, value):
        self.counter.fill_(int(value))


# ------------------------------------------------------------------------------------------------- CPU form
_M = (0xD2511F53, 0xCD9E8D57)
_W = (0x9E3779B9, 0xBB67AE85)


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al., SC'11) on uint32 arrays: ctr = 4 arrays (broadcastable), key = 2 ints -> 4
    uint32 arrays."""
    c = [np.asarray(x, np.uint32) for x in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for r in range(10):
        if r:
            k0 = (k0 + _W[0]) & 0xFFFFFFFF
            k1 = (k1 + _W[1]) & 0xFFFFFFFF
        p0 = np.uint64(_M[0]) * c[0].astype(np.uint64)
        p1 = np.uint64(_M[1]) * c[2].astype(np.uint64)
        c = [(p1 >> np.uint64(32)).astype(np.uint32) ^ c[1] ^ np.uint32(k0), p1.astype(np.uint32),
             (p0 >> np.uint64(32)).astype(np.uint32) ^ c[3] ^ np.uint32(k1), p0.astype(np.uint32)]
    return c


def _u53(a, b):
    return ((a >> np.uint32(5)).astype(np.float64) * 67108864.0 + (b >> np.uint32(6)).astype(np.float64)) / 9007199254740992.0


def point_uniforms(seed, counter, batch, n_points):
    """(batch, n_points, 6) U[0, 1) of the device draws: noise x, y, z, colour r, g, b."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    ctr = int(counter) & 0xFFFFFFFFFFFFFFFF
    n = np.arange(n_points, dtype=np.uint32)[None, :]
    b = np.arange(batch, dtype=np.uint32)[:, None]
    u = np.empty((batch, n_points, 6))
    for j in range(3):
        w = philox4x32_10((n, (b << np.uint32(2)) | np.uint32(j), ctr & 0xFFFFFFFF, ctr >> 32), (seed, seed >> 32))
        u[..., 2 * j] = _u53(w[0], w[1])
        u[..., 2 * j + 1] = _u53(w[2], w[3])
    return u


def _rot(R, x, y, z):
    R = R.reshape(-1, 9)
    r = [R[:, i:i + 1] if x.ndim == 2 else R[:, i:i + 1, None] for i in range(9)]
    return ((r[0] * x + r[1] * y) + r[2] * z, (r[3] * x + r[4] * y) + r[5] * z, (r[6] * x + r[7] * y) + r[8] * z)


def cpu_form(bank, ints, params, *, train=True, use_color=True, det_mode=0, augment_det=False, seed=0, counter=0,
             explicit=None):
    """numpy restatement of csrc/augment.hip (same operation order, same Philox draws): dict of numpy arrays."""
    slots = ints[:, I_SLOT].astype(np.int64)
    B, N = len(slots), bank.n_points
    P = params
    xyz = bank.xyz.cpu().numpy()[slots]
    color = bank.color.cpu().numpy()[slots]
    obj = bank.obj.cpu().numpy()[slots].astype(np.int64)
    x, y, z = xyz[..., 0], xyz[..., 1], xyz[..., 2]
    col = color.astype(np.float64) - MEAN_RGB
    if train:
        if explicit is not None:
            noise = np.asarray(explicit["noise"], np.float64).reshape(B, N, 3)
            cf = np.asarray(explicit["color_factor"], np.float64).reshape(B, N, 3)
        else:
            u = point_uniforms(seed, counter, B, N)
            noise = u[..., :3] * 5e-3
            cf = 0.98 + 0.04 * u[..., 3:]
        x = np.where(P[:, P_YZ:P_YZ + 1] != 0, -x, x)
        y = np.where(P[:, P_XZ:P_XZ + 1] != 0, -y, y)
        for off in (P_RZ, P_RX, P_RY):
            x, y, z = _rot(P[:, off:off + 9], x, y, z)
        x = x + noise[..., 0]
        y = y + noise[..., 1]
        z = z + noise[..., 2]
        sh, sc = P[:, P_SHIFT:P_SHIFT + 3], P[:, P_SCALE:P_SCALE + 1]
        x = x + sh[:, 0:1]
        y = y + sh[:, 1:2]
        z = z + sh[:, 2:3]
        x, y, z = x * sc, y * sc, z * sc
        col = (col + MEAN_RGB) * cf - MEAN_RGB
    pts = np.stack([x, y, z], -1)
    pc = np.concatenate([pts, col], -1) if use_color else pts
    out = {"point_clouds": pc.astype(np.float32), "og_color": color.copy()}
    n_obj = bank.max_objects
    label = np.full((B, N), -1, np.int64)
    center = np.zeros((B, ROWS, 3))
    size = np.zeros((B, ROWS, 3))
    mask = np.zeros((B, ROWS), np.float32)
    allb = np.zeros((B, ROWS, 6))
    det = np.zeros((B, ROWS, 6))
    dcls = np.zeros((B, ROWS), np.int64)
    for b in range(B):
        nt = int(ints[b, I_NT])
        tids = ints[b, I_TIDS:I_TIDS + nt].astype(np.int64)
        rank = np.full(n_obj, -1, np.int64)
        rank[tids] = np.arange(nt)                    # (a repeated id keeps its last rank, as in the reference)
        o = obj[b]
        inside = o >= 0
        label[b, inside] = rank[o[inside]]
        # per-object min / max of the augmented points
        boxes = np.zeros((n_obj, 6))
        if inside.any():
            order = np.argsort(o[inside], kind="stable")
            ids = o[inside][order]
            p = pts[b][inside][order]
            starts = np.flatnonzero(np.r_[True, ids[1:] != ids[:-1]])
            mn = np.minimum.reduceat(p, starts, axis=0)
            mx = np.maximum.reduceat(p, starts, axis=0)
            for k, oid in enumerate(ids[starts]):
                boxes[oid] = _box_cs(mn[k], mx[k])
        c = boxes[tids]
        if train:
            c = c * P[b, P_JT:P_JT + nt * 6].reshape(nt, 6)
        center[b, :nt], size[b, :nt] = c[:, :3], c[:, 3:]
        center[b, nt:] = 1000
        mask[b, :nt] = 1
        keep = ints[b, I_KEEP:I_KEEP + ROWS] != 0
        a = np.zeros((ROWS, 6))
        rows = np.flatnonzero(keep)
        a[rows] = boxes[rows]
        if train:
            a = a * P[b, P_JA:P_JA + ROWS * 6].reshape(ROWS, 6)
        allb[b] = a
        if det_mode == 1:
            w = bank.det_box[int(slots[b])].cpu().numpy().copy()
            cls = bank.det_cls[int(slots[b])].cpu().numpy().astype(np.int64)
            if train:
                lo, hi = w[:, :3] - w[:, 3:] / 2, w[:, :3] + w[:, 3:] / 2
                cx = np.stack([lo[:, 0], lo[:, 0], hi[:, 0], hi[:, 0], lo[:, 0], lo[:, 0], hi[:, 0], hi[:, 0]], 1)
                cy = np.stack([lo[:, 1], hi[:, 1], lo[:, 1], hi[:, 1], lo[:, 1], hi[:, 1], lo[:, 1], hi[:, 1]], 1)
                cz = np.stack([lo[:, 2]] * 4 + [hi[:, 2]] * 4, 1)
                for off in (P_RZ, P_RX, P_RY):
                    R = P[b, off:off + 9]
                    cx, cy, cz = ((R[0] * cx + R[1] * cy) + R[2] * cz, (R[3] * cx + R[4] * cy) + R[5] * cz,
                                  (R[6] * cx + R[7] * cy) + R[8] * cz)
                if P[b, P_YZ] != 0:
                    cx = -cx
                if P[b, P_XZ] != 0:
                    cy = -cy
                cx, cy, cz = cx + P[b, P_SHIFT], cy + P[b, P_SHIFT + 1], cz + P[b, P_SHIFT + 2]
                cx, cy, cz = cx * P[b, P_SCALE], cy * P[b, P_SCALE], cz * P[b, P_SCALE]
                corners = np.stack([cx, cy, cz], -1)
                mn, mx = corners.min(1), corners.max(1)
                w = np.concatenate(((mn + mx) / 2, mx - mn), 1)
                if augment_det:
                    mn0, mx0 = w.min(0), w.max(0)
                    rand_box = (mx0 - mn0)[None] * P[b, P_RB:P_RB + ROWS * 6].reshape(ROWS, 6) + mn0
                    corrupt = P[b, P_CR:P_CR + ROWS] > 0.7
                    w[corrupt] = rand_box[corrupt]
                    cls[corrupt] = P[b, P_RC:P_RC + ROWS].astype(np.int64)[corrupt]
            det[b], dcls[b] = w, cls
        elif det_mode == 2:
            det[b] = allb[b]
            dcls[b] = ints[b, I_DCLS:I_DCLS + ROWS]
    out.update({"center_label": center.astype(np.float32), "size_gts": size.astype(np.float32),
                "box_label_mask": mask, "point_instance_label": label, "all_bboxes": allb.astype(np.float32),
                "all_detected_boxes": det.astype(np.float32), "all_detected_class_ids": dcls})
    return out
