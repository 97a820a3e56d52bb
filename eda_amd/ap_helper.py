"""Detection mAP of EDA's ScanNet evaluation: drop-in for the reference's models/ap_helper.py.

Same public surface as the reference (`parse_predictions`, `parse_groundtruths`, `APCalculator` with `.step`,
`.compute_metrics`, `.reset`; the tuple lists, `end_points[f'{prefix}pred_mask']`, `end_points['batch_gt_map_cls']`,
the metric keys), organised for the device (csrc/det_eval.hip):

    decode      camera-frame AABB (fp64), objectness, per-class probabilities, arg-max class   one thread per proposal
    3D NMS      greedy, class-aware or not, new or old overlap                                  one workgroup per scene
    matching    first-maximum IoU against the scene's ground truth of the class, TP flags       one wave per (threshold,
                                                                                                class, scene) segment
    AP          stable sort per class, cumulative sums, VOC envelope, area   batched torch over all classes and thresholds

`parse_predictions(..., as_tensors=True)` / `parse_groundtruths(..., as_tensors=True)` return device records
(`DetPredictions`, `DetGroundTruths`); `APCalculator.step` accumulates them without leaving the GPU and
`compute_metrics` makes ONE device-to-host copy.  The tuple form (the default) is the exact drop-in: its corners are
rebuilt on the host from the AABBs, one copy per batch, and `compute_metrics` on tuples runs the CPU form.

CPU tensors take the numpy form of this module (same semantics, same fp64 arithmetic; it is the second opinion the GPU
tests compare against).

Semantics pinned by tests/golden/det_eval_*.npz (produced by running the reference):
  - boxes: flip_axis_to_camera (x, -z, y) and get_3d_box with heading 0; the size halves are fp32, widened and added to
    the fp32 centre in fp64.  Sizes are non-negative (the heads' output): the corners of a tuple are (max, max, min,
    min, ...) in the reference's vertex order.
  - NMS order: descending objectness, ties to the LARGER index (a stable ascending argsort; the reference's quicksort
    leaves ties undefined).
  - the IoU of the matching is axis-aligned: for heading-0 boxes the reference's box3d_iou (polygon clipping +
    ConvexHull) computes the same quantity, up to rounding.
  - AP order per class: descending confidence, ties in (scene, proposal) order (the reference's insertion order; its
    quicksort leaves ties undefined).
  - the class set is the union of the classes with ground truth and the classes with predictions; a class with
    predictions but no ground truth has AP 0.  ONE intended deviation: a class with ground truth but no prediction gets
    AP 0 and recall 0 (the reference misaligns its per-class results then, eval_det.py:349-356; that cannot happen with
    per_class_proposal=True).
Supported configurations are EDA's: use_3d_nms=True with cls_nms on or off, use_old_type_nms on or off,
per_class_proposal on or off, any conf_thresh, hungarian_loss with or without objectness logits, size_cls_agnostic=True.
remove_empty_box=True, 2D NMS and size-class decoding raise NotImplementedError.
"""
import numpy as np
import torch

from . import _lib

MAX_K = 1024            # proposals per scene (NMS workgroup, matching segment)
MAX_G = 1024            # ground-truth boxes per scene
_F64_EPS = np.finfo(np.float64).eps


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _check_config(config_dict, size_cls_agnostic):
    if not size_cls_agnostic:
        raise NotImplementedError("size_cls_agnostic=False (size-class decoding) is not supported")
    if config_dict.get("remove_empty_box", False):
        raise NotImplementedError("remove_empty_box=True is not supported")
    if not config_dict.get("use_3d_nms", False):
        raise NotImplementedError("use_3d_nms=False (2D NMS) is not supported")


class DetPredictions:
    """Parsed predictions of one batch (device-resident when parsed from GPU tensors).
    aabb (B, K, 6) fp64 camera frame; keep (B, K) bool NMS picks; valid (B, K) bool = keep & obj_prob > conf_thresh;
    conf (B, K, C) fp32 per-class confidences (per_class_proposal) or (B, K, 1) objectness; sem_cls (B, K) int32."""

    def __init__(self, aabb, keep, valid, conf, sem_cls, num_class, per_class):
        self.aabb, self.keep, self.valid, self.conf, self.sem_cls = aabb, keep, valid, conf, sem_cls
        self.num_class, self.per_class = int(num_class), bool(per_class)

    def __len__(self):
        return self.aabb.shape[0]


class DetGroundTruths:
    """Parsed ground truth of one batch: aabb (B, G, 6) fp64 camera frame, cls (B, G) int32 (-1 = no box)."""

    def __init__(self, aabb, cls):
        self.aabb, self.cls = aabb, cls

    def __len__(self):
        return self.aabb.shape[0]


# ---------------------------------------------------------------------------------------------------- the numpy form
def _aabb_np(center, size):
    """(..., 3) fp32 centre and size (depth frame) -> (..., 6) fp64 camera-frame AABB."""
    center = np.asarray(center, dtype=np.float32)
    size = np.asarray(size, dtype=np.float32)
    cam = np.stack([center[..., 0], -center[..., 2], center[..., 1]], -1)
    half = np.stack([size[..., 0] / 2, size[..., 2] / 2, size[..., 1] / 2], -1)          # (l, h, w) halves, fp32
    a = cam.astype(np.float64) + half.astype(np.float64)
    b = cam.astype(np.float64) + (-half).astype(np.float64)
    return np.concatenate([np.minimum(a, b), np.maximum(a, b)], -1)


def _decode_np(center, size, logits, obj_logits):
    logits = np.asarray(logits, dtype=np.float32)
    e = np.exp(logits - np.max(logits, axis=-1, keepdims=True))
    probs = e / np.sum(e, axis=-1, keepdims=True)
    if obj_logits is not None:
        obj = 1 / (1 + np.exp(-np.asarray(obj_logits, dtype=np.float32)))
        cls_prob = probs[..., :-1]
    else:
        obj = 1 - probs[..., -1]
        cls_prob = probs[..., :-1] / obj[..., None]
    sem_cls = np.argmax(logits[..., :-1], -1).astype(np.int32)
    return _aabb_np(center, size), obj.astype(np.float32), cls_prob.astype(np.float32), sem_cls


def _iou_np(a, b):
    """IoU of AABBs a (..., 6) and b (..., 6), broadcast; the kernels' operation order."""
    lo = np.maximum(a[..., :3], b[..., :3])
    hi = np.minimum(a[..., 3:], b[..., 3:])
    e = np.maximum(0, hi - lo)
    inter = e[..., 0] * e[..., 1] * e[..., 2]
    va = (a[..., 3] - a[..., 0]) * (a[..., 4] - a[..., 1]) * (a[..., 5] - a[..., 2])
    vb = (b[..., 3] - b[..., 0]) * (b[..., 4] - b[..., 1]) * (b[..., 5] - b[..., 2])
    return inter / (va + vb - inter)


def _nms_np(aabb, score, cls, iou_thresh, old_type, cls_nms):
    B, K = score.shape
    keep = np.zeros((B, K), dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore"):        # 0/0 overlaps of zero-volume boxes are NaN, as upstream
        for b in range(B):
            _nms_scene(keep[b], aabb[b], score[b], None if cls is None else cls[b], iou_thresh, old_type, cls_nms)
    return keep


def _nms_scene(keep, box, score, cls, iou_thresh, old_type, cls_nms):
    K = score.shape[0]
    x1, y1, z1, x2, y2, z2 = (box[:, k] for k in range(6))
    area = (x2 - x1) * (y2 - y1) * (z2 - z1)
    order = np.argsort(score, kind="stable")[::-1]         # descending, ties to the larger index, NaN first
    alive = np.ones(K, dtype=bool)
    for pos, i in enumerate(order):
        if not alive[i]:
            continue
        keep[i] = True
        rest = order[pos + 1:]
        rest = rest[alive[rest]]
        if rest.size == 0:
            break
        l = np.maximum(0, np.minimum(x2[i], x2[rest]) - np.maximum(x1[i], x1[rest]))
        w = np.maximum(0, np.minimum(y2[i], y2[rest]) - np.maximum(y1[i], y1[rest]))
        h = np.maximum(0, np.minimum(z2[i], z2[rest]) - np.maximum(z1[i], z1[rest]))
        inter = l * w * h
        o = inter / area[rest] if old_type else inter / (area[i] + area[rest] - inter)
        if cls_nms:
            o = o * (cls[i] == cls[rest])
        alive[rest[o > iou_thresh]] = False


def _match_np(p_scene, p_cls, p_aabb, p_conf, g_scene, g_cls, g_aabb, thresholds):
    """Flat predictions (in insertion order) and ground truth -> per class: the prediction indices in AP order and
    their TP flags (T, n) per threshold."""
    gts = {}
    for k in range(len(g_cls)):
        gts.setdefault((int(g_cls[k]), int(g_scene[k])), []).append(k)
    out = {}
    T = len(thresholds)
    for c in np.unique(p_cls):
        idx = np.flatnonzero(p_cls == c)
        order = idx[np.argsort(-p_conf[idx], kind="stable")]   # descending, ties in insertion order, NaN last
        tp = np.zeros((T, order.size), dtype=bool)
        sc = p_scene[order]
        for s in np.unique(sc):
            g = gts.get((int(c), int(s)))
            if not g:
                continue
            pos = np.flatnonzero(sc == s)
            with np.errstate(invalid="ignore", divide="ignore"):
                ious = _iou_np(p_aabb[order[pos]][:, None, :], g_aabb[g][None, :, :])   # (P, G)
            for t, thr in enumerate(thresholds):
                taken = np.zeros(len(g), dtype=bool)
                for r, row in zip(pos, ious):
                    ok = row == row
                    if not ok.any():
                        continue
                    m = row[ok].max()
                    if not m > thr:
                        continue
                    jm = int(np.flatnonzero(row == m)[0])
                    if not taken[jm]:
                        taken[jm] = True
                        tp[t, r] = True
        out[c] = (order, tp)
    return out


def _voc_ap_np(rec, prec):
    mrec = np.concatenate(([0.0], rec, [1.0]))
    mpre = np.concatenate(([0.0], prec, [0.0]))
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]
    i = np.flatnonzero(mrec[1:] != mrec[:-1])
    return np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])


def _metrics_np(p_scene, p_cls, p_aabb, p_conf, g_scene, g_cls, g_aabb, thresholds):
    """-> per threshold: ({cls: ap}, {cls: recall}) over the class set (gt classes | predicted classes)."""
    matched = _match_np(p_scene, p_cls, p_aabb, p_conf, g_scene, g_cls, g_aabb, thresholds)
    classes = sorted(set(int(c) for c in np.unique(g_cls)) | set(int(c) for c in matched))
    npos = {c: int(np.sum(g_cls == c)) for c in classes}
    res = []
    for t in range(len(thresholds)):
        ap, rec = {}, {}
        for c in classes:
            if c not in matched:
                ap[c], rec[c] = 0.0, 0.0
                continue
            tpf = matched[c][1][t].astype(np.float64)
            tpc = np.cumsum(tpf)
            fpc = np.cumsum(1.0 - tpf)
            r = tpc / float(npos[c] + 1e-8)
            p = tpc / np.maximum(tpc + fpc, _F64_EPS)
            ap[c] = float(_voc_ap_np(r, p))
            rec[c] = float(r[-1])
        res.append((ap, rec))
    return res


# ------------------------------------------------------------------------------------------------- explicit entries
def nms_3d(aabb, score, cls, iou_thresh, old_type=False, cls_nms=True):
    """Greedy 3D NMS per scene.  aabb (B, K, 6) fp64, score (B, K) fp64, cls (B, K) int (may be None without cls_nms)
    -> keep (B, K) bool.  GPU tensors run eda_det_nms_f64; numpy arrays / CPU tensors the numpy form."""
    if isinstance(aabb, torch.Tensor) and aabb.is_cuda:
        B, K = score.shape
        if K > MAX_K:
            raise ValueError(f"nms_3d: K = {K} > {MAX_K}")
        aabb = aabb.to(torch.float64).contiguous()
        score = score.to(torch.float64).contiguous()
        cls_t = cls.to(torch.int32).contiguous() if cls is not None else None
        keep = torch.empty(B, K, dtype=torch.uint8, device=aabb.device)
        _lib.check(_lib.lib().eda_det_nms_f64(aabb.data_ptr(), score.data_ptr(), _ptr(cls_t), B, K, float(iou_thresh),
                                              int(bool(old_type)), int(bool(cls_nms)), keep.data_ptr(), _stream()),
                   "eda_det_nms_f64")
        return keep.bool()
    to_np = (lambda x: x.numpy() if isinstance(x, torch.Tensor) else np.asarray(x))
    keep = _nms_np(to_np(aabb).astype(np.float64), to_np(score).astype(np.float64),
                   None if cls is None else to_np(cls), float(iou_thresh), old_type, cls_nms)
    return torch.from_numpy(keep) if isinstance(aabb, torch.Tensor) else keep


def match_tp(pred_aabb, conf, pred_cls, pred_valid, gt_aabb, gt_cls, thresholds, num_class):
    """AP matching on the device (eda_det_match_f64).  pred_aabb (S, K, 6) fp64; conf (S, K, C) per-class or (S, K, 1)
    fp64 confidences; pred_cls (S, K) int: the class of each prediction, or None = every class (per-class proposals);
    pred_valid (S, K) bool; gt_aabb (S, G, 6) fp64; gt_cls (S, G) int, -1 = no box -> tp (T, C, S, K) bool."""
    S, K = pred_valid.shape
    G = gt_cls.shape[1]
    if K > MAX_K or G > MAX_G:
        raise ValueError(f"match_tp: K = {K}, G = {G} (at most {MAX_K}, {MAX_G})")
    dev = pred_aabb.device
    thr = torch.as_tensor(list(thresholds), dtype=torch.float64).to(dev)
    T = thr.numel()
    pred_aabb = pred_aabb.to(torch.float64).contiguous()
    conf = conf.to(torch.float64).contiguous()
    pcls = pred_cls.to(torch.int32).contiguous() if pred_cls is not None else None
    pvalid = pred_valid.to(torch.uint8).contiguous()
    gt_aabb = gt_aabb.to(torch.float64).contiguous()
    gcls = gt_cls.to(torch.int32).contiguous()
    tp = torch.empty(T, num_class, S, K, dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib().eda_det_match_f64(pred_aabb.data_ptr(), conf.data_ptr(), conf.shape[-1], _ptr(pcls),
                                            pvalid.data_ptr(), gt_aabb.data_ptr() if G else None,
                                            gcls.data_ptr() if G else None, thr.data_ptr(), S, K, G, num_class, T,
                                            tp.data_ptr(), _stream()),
               "eda_det_match_f64")
    return tp.bool()


def ap_from_tp(tp, conf, pred_cls, pred_valid, gt_cls, num_class):
    """Batched AP reduction on the device: tp (T, C, S, K) from match_tp, the same conf / pred_cls / pred_valid, gt_cls
    (S, G) -> ap (T, C), recall (T, C), in_set (C) (the class has ground truth or predictions), all on the device."""
    T, C, S, K = tp.shape
    N = S * K
    dev = tp.device
    valid = pred_valid.reshape(1, N).bool()
    if pred_cls is None:
        ispred = valid.expand(C, N)
        confT = conf.reshape(N, C).t().to(torch.float64)
    else:
        ispred = valid & (pred_cls.reshape(1, N).long() == torch.arange(C, device=dev)[:, None])
        confT = conf.reshape(1, N).to(torch.float64).expand(C, N)
    key = torch.where(ispred, -confT, torch.zeros((), dtype=torch.float64, device=dev))
    o1 = torch.sort(key, dim=1, stable=True).indices              # descending confidence, ties by (scene, j), NaN last
    o2 = torch.sort((~ispred).gather(1, o1).to(torch.uint8), dim=1, stable=True).indices   # predictions first
    perm = o1.gather(1, o2)
    isp = ispred.gather(1, perm)                                  # (C, N): a prefix of True
    tps = tp.reshape(T, C, N).gather(2, perm[None].expand(T, C, N)).to(torch.float64)
    tpc = torch.cumsum(tps, -1)
    fpc = torch.cumsum(isp[None].to(torch.float64) - tps, -1)
    npos = (gt_cls.reshape(-1, 1).long() == torch.arange(C, device=dev)[None, :]).sum(0).to(torch.float64)
    rec = tpc / (npos + 1e-8)[None, :, None]
    prec = tpc / torch.clamp(tpc + fpc, min=_F64_EPS)
    z = torch.zeros(T, C, 1, dtype=torch.float64, device=dev)
    mrec = torch.cat([z, torch.where(isp[None], rec, 1.0), z + 1.0], -1)
    mpre = torch.cat([z, torch.where(isp[None], prec, 0.0), z], -1)
    mpre = torch.flip(torch.cummax(torch.flip(mpre, [-1]), -1).values, [-1])
    d = mrec[..., 1:] - mrec[..., :-1]
    ap = torch.where(d != 0, d * mpre[..., 1:], 0.0).sum(-1)
    nd = isp.sum(-1)                                              # (C,)
    last = torch.gather(rec, 2, (nd - 1).clamp(min=0)[None, :, None].expand(T, C, 1))[..., 0]
    recall = torch.where(nd[None] > 0, last, 0.0)
    in_set = (npos > 0) | (nd > 0)
    return ap, recall, in_set


# ----------------------------------------------------------------------------------------------- reference surface
def _end_point(end_points, key):
    t = end_points[key]
    return t.detach() if isinstance(t, torch.Tensor) else torch.as_tensor(t)


def parse_predictions(end_points, config_dict, prefix="", size_cls_agnostic=False, as_tensors=False):
    """Decode the proposals of `prefix`, suppress overlapping boxes (3D NMS) and return
    the reference's lists [[(cls, corners (8, 3) fp64, score), ...] per scene] (scene, then class-major, then j), or
    with as_tensors=True a DetPredictions record on the tensors' device.  In the cls_nms branch
    end_points[f'{prefix}pred_mask'] is set: a (B, K) float64 numpy array (a device tensor with as_tensors=True)."""
    _check_config(config_dict, size_cls_agnostic)
    center = _end_point(end_points, f"{prefix}center").to(torch.float32)
    size = _end_point(end_points, f"{prefix}pred_size").to(torch.float32)
    logits = _end_point(end_points, f"{prefix}sem_cls_scores").to(torch.float32)
    B, K = center.shape[:2]
    C1 = logits.shape[-1]
    C = C1 - 1
    if config_dict.get("hungarian_loss", False):
        okey = f"{prefix}objectness_scores"
        obj_logits = _end_point(end_points, okey).to(torch.float32).reshape(B, K) if okey in end_points else None
    else:
        obj_logits = _end_point(end_points, f"{prefix}objectness_scores").to(torch.float32).reshape(B, K)
    cls_nms = bool(config_dict.get("cls_nms", False))
    old_type = bool(config_dict.get("use_old_type_nms", False))
    per_class = bool(config_dict["per_class_proposal"])
    conf_thresh = float(np.float32(config_dict["conf_thresh"]))
    if center.is_cuda:
        if K > MAX_K:
            raise ValueError(f"parse_predictions: K = {K} > {MAX_K}")
        dev = center.device
        center, size, logits = center.contiguous(), size.contiguous(), logits.contiguous()
        obj_logits = obj_logits.contiguous() if obj_logits is not None else None
        aabb = torch.empty(B, K, 6, dtype=torch.float64, device=dev)
        obj = torch.empty(B, K, dtype=torch.float32, device=dev)
        cls_prob = torch.empty(B, K, C, dtype=torch.float32, device=dev)
        sem_cls = torch.empty(B, K, dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().eda_det_decode_f32(center.data_ptr(), size.data_ptr(), logits.data_ptr(),
                                                 _ptr(obj_logits), B, K, C1, aabb.data_ptr(), obj.data_ptr(),
                                                 cls_prob.data_ptr(), sem_cls.data_ptr(), _stream()),
                   "eda_det_decode_f32")
        keep = nms_3d(aabb, obj.to(torch.float64), sem_cls, config_dict["nms_iou"], old_type, cls_nms)
    else:
        aabb, obj, cls_prob, sem_cls = _decode_np(center.numpy(), size.numpy(), logits.numpy(),
                                                  None if obj_logits is None else obj_logits.numpy())
        keep = _nms_np(aabb, obj.astype(np.float64), sem_cls, float(config_dict["nms_iou"]), old_type, cls_nms)
        aabb, obj, cls_prob, sem_cls, keep = (torch.from_numpy(x) for x in (aabb, obj, cls_prob, sem_cls, keep))
    valid = keep & (obj > conf_thresh)
    conf = cls_prob * obj[..., None] if per_class else obj[..., None]
    rec = DetPredictions(aabb, keep, valid, conf, sem_cls, C, per_class)
    if as_tensors:
        if cls_nms:
            end_points[f"{prefix}pred_mask"] = keep.to(torch.float64)
        return rec
    # the one copy of this batch: [aabb | keep | valid | sem_cls | conf]
    h = torch.cat([aabb, keep[..., None].double(), valid[..., None].double(), sem_cls[..., None].double(),
                   conf.double()], -1).cpu().numpy()
    corners = _corners_np(h[..., :6])
    keep_h, valid_h = h[..., 6] == 1, h[..., 7] == 1
    sem_h = h[..., 8].astype(np.int64)
    conf_h = h[..., 9:].astype(np.float32)
    if cls_nms:
        end_points[f"{prefix}pred_mask"] = keep_h.astype(np.float64)
    out = []
    for i in range(B):
        js = np.flatnonzero(valid_h[i])
        if per_class:
            out.append([(ii, corners[i, j], conf_h[i, j, ii]) for ii in range(C) for j in js])
        else:
            out.append([(int(sem_h[i, j]), corners[i, j], conf_h[i, j, 0]) for j in js])
    return out


def _corners_np(aabb):
    """(..., 6) AABBs -> (..., 8, 3) corners in get_3d_box's vertex order (heading 0, non-negative sizes)."""
    x1, y1, z1, x2, y2, z2 = (aabb[..., k] for k in range(6))
    xs = np.stack([x2, x2, x1, x1, x2, x2, x1, x1], -1)
    ys = np.stack([y2, y2, y2, y2, y1, y1, y1, y1], -1)
    zs = np.stack([z2, z1, z1, z2, z2, z1, z1, z2], -1)
    return np.stack([xs, ys, zs], -1)


def parse_groundtruths(end_points, config_dict, size_cls_agnostic, as_tensors=False):
    """Ground-truth boxes: the reference's lists [[(cls, corners (8, 3) fp64), ...] per scene], or with as_tensors=True
    a DetGroundTruths record on the tensors' device.  end_points['batch_gt_map_cls'] is set to what is returned."""
    if not size_cls_agnostic:
        raise NotImplementedError("size_cls_agnostic=False (size-class decoding) is not supported")
    center = _end_point(end_points, "center_label")[:, :, 0:3].to(torch.float32)
    size = _end_point(end_points, "size_gts").to(torch.float32)
    mask = _end_point(end_points, "box_label_mask")
    label = _end_point(end_points, "sem_cls_label")
    B, G = center.shape[:2]
    cam = torch.stack([center[..., 0], -center[..., 2], center[..., 1]], -1)
    half = torch.stack([size[..., 0] / 2, size[..., 2] / 2, size[..., 1] / 2], -1)
    a = cam.double() + half.double()
    b = cam.double() + (-half).double()
    aabb = torch.cat([torch.minimum(a, b), torch.maximum(a, b)], -1)
    cls = torch.where(mask == 1, label.to(torch.int64), -1).to(torch.int32)
    if as_tensors:
        rec = DetGroundTruths(aabb, cls)
        end_points["batch_gt_map_cls"] = rec
        return rec
    h = torch.cat([aabb, cls[..., None].double()], -1).cpu().numpy()
    corners = _corners_np(h[..., :6])
    out = [[(int(h[i, j, 6]), corners[i, j]) for j in np.flatnonzero(h[i, :, 6] >= 0)] for i in range(B)]
    end_points["batch_gt_map_cls"] = out
    return out


def det_class_scores(end_points, word_idx, token_idx, prefix="last_"):
    """Class scores of the contrastive head (the glue of the reference's ScanNet detection loop): proj_queries .
    proj_tokens^T / 0.07, zero-padded to 256 token columns, token columns summed into max(word_idx) + 1 class columns
    (in the order of the (word, token) pairs).  Stores end_points[f'{prefix}sem_cls_scores'] and returns it."""
    word_idx = [int(w) for w in word_idx]
    token_idx = [int(t) for t in token_idx]
    pt = end_points["proj_tokens"]
    pq = end_points[f"{prefix}proj_queries"]
    s = torch.matmul(pq, pt.transpose(-1, -2)) / 0.07
    B, Q, T = s.shape
    padded = s.new_zeros(B, Q, max(256, T))
    padded[:, :, :T] = s
    W = max(word_idx) + 1
    lists = [[t for w, t in zip(word_idx, token_idx) if w == k] for k in range(W)]
    M = max(len(x) for x in lists)
    zcol = padded.shape[-1]                                      # index of an appended zero column
    src = torch.cat([padded, padded.new_zeros(B, Q, 1)], -1)
    idx = torch.tensor([x + [zcol] * (M - len(x)) for x in lists], device=s.device)   # (W, M)
    out = padded.new_zeros(B, Q, W)
    for m in range(M):                                           # the reference's accumulation order, word by word
        out = out + src[..., idx[:, m]]
    end_points[f"{prefix}sem_cls_scores"] = out
    return out


def _pad(t, dim, n, value):
    if t.shape[dim] == n:
        return t
    shape = list(t.shape)
    shape[dim] = n - t.shape[dim]
    return torch.cat([t, t.new_full(shape, value)], dim)


class APCalculator:
    """Average precision over accumulated batches (reference: models/ap_helper.py APCalculator)."""

    def __init__(self, ap_iou_thresh=0.25, class2type_map=None):
        self.ap_iou_thresh = ap_iou_thresh
        self.class2type_map = class2type_map
        self.uniq_gt_classes = set()
        self.reset()

    def step(self, batch_pred_map_cls, batch_gt_map_cls):
        """Accumulate one batch: the tuple lists of parse_predictions / parse_groundtruths, or their records."""
        if isinstance(batch_pred_map_cls, DetPredictions) != isinstance(batch_gt_map_cls, DetGroundTruths):
            raise TypeError("APCalculator.step: predictions and ground truth must both be records or both be lists")
        bsize = len(batch_pred_map_cls)
        assert bsize == len(batch_gt_map_cls)
        if isinstance(batch_pred_map_cls, DetPredictions):
            if self.pred_map_cls:
                raise TypeError("APCalculator.step: records cannot follow tuple lists (reset first)")
            self.records.append((batch_pred_map_cls, batch_gt_map_cls))
            self.scan_cnt += bsize
            return
        if self.records:
            raise TypeError("APCalculator.step: tuple lists cannot follow records (reset first)")
        for i in range(bsize):
            self.gt_map_cls[self.scan_cnt] = batch_gt_map_cls[i]
            for classname, _ in batch_gt_map_cls[i]:
                self.uniq_gt_classes.add(classname)
            self.pred_map_cls[self.scan_cnt] = batch_pred_map_cls[i]
            self.scan_cnt += 1

    def _names(self, key):
        return self.class2type_map[key] if self.class2type_map else str(key)

    def _ret_dict(self, ap, rec):
        ret = {}
        keys = sorted(ap.keys())
        for k in keys:
            ret["%s Average Precision" % self._names(k)] = ap[k]
        ret["mAP"] = float(np.mean([ap[k] for k in keys])) if keys else float("nan")
        for k in keys:
            ret["%s Recall" % self._names(k)] = rec[k]
        ret["AR"] = float(np.mean([rec[k] for k in keys])) if keys else float("nan")
        return ret

    def compute_metrics(self):
        """{'<name> Average Precision', 'mAP', '<name> Recall', 'AR'} at self.ap_iou_thresh."""
        return self.compute_metrics_at([self.ap_iou_thresh])[0]

    def compute_metrics_at(self, thresholds):
        """compute_metrics for several IoU thresholds over the same accumulated batches: one matching launch and one
        device-to-host copy for all of them on the record path.  Returns one dict per threshold."""
        thresholds = [float(t) for t in thresholds]
        if self.records and self.records[0][0].aabb.is_cuda:
            return self._metrics_device(thresholds)
        p_scene, p_cls, p_aabb, p_conf, g_scene, g_cls, g_aabb = self._flat_host()
        res = _metrics_np(p_scene, p_cls, p_aabb, p_conf, g_scene, g_cls, g_aabb, thresholds)
        return [self._ret_dict(ap, rec) for ap, rec in res]

    def _flat_host(self):
        """Flat prediction / ground-truth arrays in insertion order (scene, then list order)."""
        ps, pc, pb, pf, gs, gc, gb = [], [], [], [], [], [], []
        if self.records:
            s0 = 0
            for pr, gr in self.records:
                B = len(pr)
                aabb, valid, conf = pr.aabb.cpu().numpy(), pr.valid.cpu().numpy(), pr.conf.cpu().numpy()
                sem = pr.sem_cls.cpu().numpy()
                for i in range(B):
                    js = np.flatnonzero(valid[i])
                    if pr.per_class:
                        C = conf.shape[-1]
                        ps += [s0 + i] * (C * js.size)
                        pc += [c for c in range(C) for _ in js]
                        pb += [aabb[i, j] for _ in range(C) for j in js]
                        pf += [conf[i, j, c] for c in range(C) for j in js]
                    else:
                        ps += [s0 + i] * js.size
                        pc += [int(sem[i, j]) for j in js]
                        pb += [aabb[i, j] for j in js]
                        pf += [conf[i, j, 0] for j in js]
                ga, gcl = gr.aabb.cpu().numpy(), gr.cls.cpu().numpy()
                for i in range(B):
                    js = np.flatnonzero(gcl[i] >= 0)
                    gs += [s0 + i] * js.size
                    gc += [int(gcl[i, j]) for j in js]
                    gb += [ga[i, j] for j in js]
                s0 += B
        else:
            for s, preds in self.pred_map_cls.items():
                for c, box, score in preds:
                    box = np.asarray(box, dtype=np.float64)
                    ps.append(s)
                    pc.append(c)
                    pb.append(np.concatenate([box.min(0), box.max(0)]))
                    pf.append(score)
            for s, gts in self.gt_map_cls.items():
                for c, box in gts:
                    box = np.asarray(box, dtype=np.float64)
                    gs.append(s)
                    gc.append(c)
                    gb.append(np.concatenate([box.min(0), box.max(0)]))
        arr = (lambda x, dt: np.asarray(x, dtype=dt))
        return (arr(ps, np.int64), arr(pc, np.int64), arr(pb, np.float64).reshape(-1, 6), arr(pf, np.float64),
                arr(gs, np.int64), arr(gc, np.int64), arr(gb, np.float64).reshape(-1, 6))

    def _metrics_device(self, thresholds):
        preds = [p for p, _ in self.records]
        gts = [g for _, g in self.records]
        per_class = preds[0].per_class
        C = preds[0].num_class
        if any(p.per_class != per_class or p.num_class != C for p in preds):
            raise ValueError("APCalculator: batches parsed with different per_class_proposal / class counts")
        K = max(p.aabb.shape[1] for p in preds)
        G = max(max(g.aabb.shape[1] for g in gts), 1)
        aabb = torch.cat([_pad(p.aabb, 1, K, 0.0) for p in preds])
        valid = torch.cat([_pad(p.valid, 1, K, False) for p in preds])
        conf = torch.cat([_pad(p.conf, 1, K, 0.0) for p in preds])
        pcls = None if per_class else torch.cat([_pad(p.sem_cls, 1, K, 0) for p in preds])
        g_aabb = torch.cat([_pad(g.aabb, 1, G, 0.0) for g in gts])
        g_cls = torch.cat([_pad(g.cls, 1, G, -1) for g in gts])
        tp = match_tp(aabb, conf, pcls, valid, g_aabb, g_cls, thresholds, C)
        ap, rec, in_set = ap_from_tp(tp, conf, pcls, valid, g_cls, C)
        bad = (g_cls >= C).any().double().reshape(1)
        h = torch.cat([ap.flatten(), rec.flatten(), in_set.double(), bad]).cpu().numpy()   # the one copy
        if h[-1]:
            raise ValueError(f"APCalculator: a ground-truth class is outside the {C} predicted classes")
        T = len(thresholds)
        ap_h = h[:T * C].reshape(T, C)
        rec_h = h[T * C:2 * T * C].reshape(T, C)
        classes = [c for c in range(C) if h[2 * T * C + c]]
        return [self._ret_dict({c: float(ap_h[t, c]) for c in classes}, {c: float(rec_h[t, c]) for c in classes})
                for t in range(T)]

    def reset(self):
        self.gt_map_cls = {}
        self.pred_map_cls = {}
        self.records = []
        self.scan_cnt = 0
