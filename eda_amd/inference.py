"""Inference: from the model's outputs to boxes, the evaluation counters on the device, the captured forward-only step and
the "give me the box" call.

    decode_grounding          end_points -> the top-k queries per object with scores, boxes and IoUs, for several prediction
                              heads and both alignments in ONE launch (csrc/ground_decode.hip)
    DeviceGroundingEvaluator  the counters of GroundingEvaluator (same keys, same numbers) kept ON the device:
                              evaluate_all() is one launch for every head and both alignments, no host synchronisation,
                              capturable; the counters are read back when dets / gts / print_stats() are asked for
    PipelinedEvalStep         the forward-only sibling of pipeline.PipelinedTrainStep: point graph | rest graph on the main
                              stream, next batch's copy + geometry + text encoder on the side stream
    GroundingSession          session.ground(point_cloud, sentences): one scene, U sentences, the point backbone once

Reference: src/grounding_evaluator.py:139-372 (what the decode computes), main_utils.py:530-566 (_main_eval_branch, the
loop PipelinedEvalStep + DeviceGroundingEvaluator replace).  CUDA tensors take the kernel (a missing kernel is an error);
CPU tensors take the torch form below -- the evaluator's fp32 arithmetic with a stable ranking -- which is what the GPU
tests compare the kernel with.
"""
import ctypes

import torch

from . import _lib
from .grounding_evaluator import GroundingEvaluator, _iou3d_pairs
from .losses import box_cxcyczwhd_to_xyzxyz
from .pipeline import _flat, _packed_like, _rebuild, _side_stream

ALIGNMENTS = ("position", "semantic")          # "bbs", "bbf" of the evaluator's keys
_MODE = {"position": "bbs", "semantic": "bbf"}
_AUX = ("modify_positive_map", "pron_positive_map", "rel_positive_map", "other_entity_map")
_FLAGS = ("is_view_dep", "is_hard", "is_unique")
_N_ANALYSIS = 2 * 3 * 2 * 2                    # [threshold 0, 1][vd, hard, unique][on, off][found, count]


def _alignments(alignment):
    if alignment is None:
        return list(ALIGNMENTS)
    names = [alignment] if isinstance(alignment, str) else list(alignment)
    assert names and all(a in ALIGNMENTS for a in names), alignment
    return [a for a in ALIGNMENTS if a in names]


def token_scores(end_points, prefix, alignment, width):
    """(B, Q, width) token probabilities of one head: the evaluator's arithmetic (grounding_evaluator.py:99-115)."""
    if alignment == "position":
        sm = end_points[f"{prefix}sem_cls_scores"].softmax(-1)
    else:
        sim = torch.matmul(end_points[f"{prefix}proj_queries"], end_points["proj_tokens"].transpose(-1, -2))
        sm = (sim / 0.07).softmax(-1)
    if sm.shape[-1] == width:
        return sm
    out = sm.new_zeros(sm.shape[0], sm.shape[1], width)
    out[:, :, :sm.shape[-1]] = sm
    return out


def query_scores(sem, targets, only_root=False):
    """(B, G, Q) score of every query for every object from token probabilities sem (B, Q, T): main map + the first
    object's modifier + pronoun + relation - other-entity maps (grounding_evaluator.py:120-133)."""
    pmap = (targets["positive_map"] > 0).to(sem.dtype)
    if only_root:
        pmap = pmap[:, :1]
    scores = torch.einsum("bqt,bot->boq", sem, pmap)
    if all(k in targets for k in _AUX):
        extra = (targets["modify_positive_map"][:, 0] + targets["pron_positive_map"][:, 0]
                 + targets["rel_positive_map"][:, 0] - targets["other_entity_map"][:, 0]).to(sem.dtype)
        scores = scores + torch.einsum("bqt,bt->bq", sem, extra)[:, None, :]
    return scores


def detected_box_gate(end_points, prefix, boxes, mask):
    """(B, Q) 1 where the head's box overlaps a masked detected box by more than 0.25 (grounding_evaluator.py:135-140)."""
    pred_c = box_cxcyczwhd_to_xyzxyz(torch.cat([end_points[f"{prefix}center"], end_points[f"{prefix}pred_size"]], -1))
    iou_d = _iou3d_pairs(box_cxcyczwhd_to_xyzxyz(boxes)[:, :, None, :], pred_c[:, None, :, :])
    iou_d = torch.where(mask.bool()[:, :, None], iou_d, iou_d.new_full((), -1.0))
    return (iou_d.max(1)[0] > 0.25).to(pred_c.dtype)


def _has_gt(tg):
    return tg is not None and "center_label" in tg and "size_gts" in tg


def _decode_torch(ep, tg, prefixes, aligns, K, only_root, gate, with_gt):
    """The torch form of the decode (any device): same outputs as the kernel.  Ranking: descending score, lowest query
    index first among equal scores (a stable sort)."""
    B, Q = ep[f"{prefixes[0]}center"].shape[:2]
    T = tg["positive_map"].shape[-1]
    G = 1 if only_root else tg["positive_map"].shape[1]
    dev = ep[f"{prefixes[0]}center"].device
    shape = (len(prefixes), len(aligns), B, G, K)
    out = {"top_query": torch.full(shape, -1, dtype=torch.int32, device=dev),
           "top_score": torch.zeros(shape, device=dev), "top_box": torch.zeros(shape + (6,), device=dev),
           "top_corners": torch.zeros(shape + (6,), device=dev)}
    if with_gt:
        out["top_iou"] = torch.zeros(shape, device=dev)
        gt = torch.cat([tg["center_label"][:, :G, 0:3], tg["size_gts"][:, :G]], -1).float()
        gt_c = box_cxcyczwhd_to_xyzxyz(gt)
    k = min(K, Q)
    for pi, p in enumerate(prefixes):
        pred = torch.cat([ep[f"{p}center"], ep[f"{p}pred_size"]], -1).float()
        pred_c = box_cxcyczwhd_to_xyzxyz(pred)
        keep = detected_box_gate(ep, p, gate[0], gate[1]) if gate is not None else None
        for ai, a in enumerate(aligns):
            scores = query_scores(token_scores(ep, p, a, T).float(), tg, only_root)
            if keep is not None:
                scores = scores * keep[:, None, :]
            s, top = torch.sort(scores, dim=-1, descending=True, stable=True)
            s, top = s[..., :k], top[..., :k]
            out["top_query"][pi, ai, ..., :k] = top.int()
            out["top_score"][pi, ai, ..., :k] = s
            idx = top[..., None].expand(B, G, k, 6)
            out["top_box"][pi, ai, :, :, :k] = torch.gather(pred[:, None].expand(B, G, Q, 6), 2, idx)
            pbox = torch.gather(pred_c[:, None].expand(B, G, Q, 6), 2, idx)
            out["top_corners"][pi, ai, :, :, :k] = pbox
            if with_gt:
                out["top_iou"][pi, ai, ..., :k] = _iou3d_pairs(gt_c[:, :, None, :], pbox)
    return out


def _f32(t):
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.float().contiguous()


def _u8(t, dev, n):
    """Flags / masks as bytes on the device (a bool tensor already there is re-viewed, not copied)."""
    t = torch.as_tensor(t, device=dev)
    if t.dtype != torch.bool:
        t = t != 0
    t = t.reshape(n) if t.numel() == n else t
    return t.contiguous().view(torch.uint8)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _table(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _decode_kernel(ep, tg, prefixes, aligns, K, only_root, gate, with_gt, outputs=True, counters=None, thresholds=(),
                   topks=(), last_prefix=-1):
    """One launch of eda_ground_decode_f32 on the current stream.  Returns the dict of outputs (or {} with outputs=False)."""
    P = len(prefixes)
    center = [_f32(ep[f"{p}center"]) for p in prefixes]
    size = [_f32(ep[f"{p}pred_size"]) for p in prefixes]
    B, Q = center[0].shape[:2]
    dev = center[0].device
    pmap = _f32(tg["positive_map"])
    Gs, T = pmap.shape[1:]
    G = 1 if only_root else Gs
    mask = (1 if "position" in aligns else 0) | (2 if "semantic" in aligns else 0)
    sem = pq = tokens = None
    Ts = L = D = 0
    if mask & 1:
        sem = [_f32(ep[f"{p}sem_cls_scores"]) for p in prefixes]
        Ts = sem[0].shape[-1]
    if mask & 2:
        pq = [_f32(ep[f"{p}proj_queries"]) for p in prefixes]
        tokens = _f32(ep["proj_tokens"])
        L, D = tokens.shape[1:]
    aux = [_f32(tg[k]) for k in _AUX] if all(k in tg for k in _AUX) else [None] * 4
    assert all(a is None or a.shape == pmap.shape for a in aux), "the auxiliary maps have the positive map's shape"
    gt_c = gt_s = lab = None
    gt_stride = 3
    if with_gt:
        gt_c, gt_s = _f32(tg["center_label"]), _f32(tg["size_gts"])
        gt_stride = gt_c.shape[-1]
        assert gt_c.shape[1] == Gs and gt_s.shape[1:] == (Gs, 3)
        if "box_label_mask" in tg:
            lab = _f32(tg["box_label_mask"])
    det = dmask = None
    Dn = 0
    if gate is not None:
        det = _f32(gate[0])
        Dn = det.shape[1]
        dmask = _u8(gate[1], dev, B * Dn)
    flags = [None] * 3
    if counters is not None and last_prefix >= 0 and all(k in tg for k in _FLAGS):
        flags = [_u8(tg[k], dev, B) for k in _FLAGS]
    out = {}
    if outputs:
        shape = (P, len(aligns), B, G, K)
        out = {"top_query": torch.empty(shape, dtype=torch.int32, device=dev), "top_score": torch.empty(shape, device=dev),
               "top_box": torch.empty(shape + (6,), device=dev), "top_corners": torch.empty(shape + (6,), device=dev)}
        if with_gt:
            out["top_iou"] = torch.empty(shape, device=dev)
    thr = (ctypes.c_float * max(len(thresholds), 1))(*thresholds)
    tk = (ctypes.c_int * max(len(topks), 1))(*topks)
    L_ = _lib.lib()
    if not L_.eda_ground_decode_supported(Q, T, G):
        raise _lib.EdaHipError(f"eda_ground_decode_f32: Q = {Q}, T = {T}, G = {G} do not fit the kernel's LDS")
    with torch.cuda.device(dev):
        rc = L_.eda_ground_decode_f32(
            P, _table(sem) if sem else None, _table(pq) if pq else None, _table(center), _table(size), _ptr(tokens),
            pmap.data_ptr(), _ptr(aux[0]), _ptr(aux[1]), _ptr(aux[2]), _ptr(aux[3]), _ptr(gt_c), gt_stride, _ptr(gt_s),
            _ptr(lab), _ptr(det), _ptr(dmask), _ptr(flags[0]), _ptr(flags[1]), _ptr(flags[2]), B, Q, Ts, L, D, T, Gs, G, Dn,
            mask, K, len(thresholds), thr, len(topks), tk, last_prefix, _ptr(out.get("top_query")),
            _ptr(out.get("top_score")), _ptr(out.get("top_box")), _ptr(out.get("top_corners")), _ptr(out.get("top_iou")),
            _ptr(counters), torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "eda_ground_decode_f32")
    return out


def _gate_of(end_points, targets, filter_non_gt_boxes):
    if not filter_non_gt_boxes:
        return None
    for d in (end_points, targets or {}):
        if "all_detected_boxes" in d:
            return d["all_detected_boxes"], d["all_detected_bbox_label_mask"]
    raise KeyError("filter_non_gt_boxes needs all_detected_boxes / all_detected_bbox_label_mask")


def decode_grounding(end_points, prefixes=("last_",), topk=10, targets=None, filter_non_gt_boxes=False, *,
                     only_root=False, alignment=None):
    """The top `topk` queries of every object, for the heads `prefixes` and the alignments (`alignment`: None = both,
    position first; "position"; "semantic"), ranked by descending score, lowest query index first among equal scores.

    Token weights, and with `targets` the ground truth, come from `targets` (positive_map (B, G, T); optionally
    modify_positive_map / pron_positive_map / rel_positive_map / other_entity_map; center_label, size_gts,
    box_label_mask); without `targets`, end_points["positive_map"] gives the token weights and no IoU is returned.
    only_root: the first object only.  Returns tensors of shape (P, A, B, G, topk[, 6]): top_query (int32, -1 beyond the
    number of queries), top_score, top_box (centre, size), top_corners (min, max) and, with targets, top_iou.
    CUDA tensors: one launch of eda_ground_decode_f32; CPU tensors: the torch form."""
    prefixes = list(prefixes)
    tg = targets if targets is not None else {"positive_map": end_points["positive_map"]}
    with_gt = targets is not None and _has_gt(targets)
    aligns = _alignments(alignment)
    gate = _gate_of(end_points, targets, filter_non_gt_boxes)
    fn = _decode_kernel if end_points[f"{prefixes[0]}center"].is_cuda else _decode_torch
    return fn(end_points, tg, prefixes, aligns, int(topk), only_root, gate, with_gt)


class DeviceGroundingEvaluator:
    """GroundingEvaluator (same constructor, same `dets` / `gts` keys and numbers) with the counters on the device.

    evaluate_all(end_points) scores every prefix under both alignments in one launch and adds into an int64 counter
    tensor with atomics: no host synchronisation, no allocation after the first call, capturable in a HIP graph.
    `dets`, `gts`, print_stats() and synchronize_between_processes() read the counters back (one copy)."""

    ANALYSIS = GroundingEvaluator.ANALYSIS

    def __init__(self, only_root=True, thresholds=(0.25, 0.5), topks=(1, 5, 10), prefixes=(), filter_non_gt_boxes=False):
        self.only_root = only_root
        self.thresholds = list(thresholds)
        self.topks = list(topks)
        self.prefixes = list(prefixes)
        self.filter_non_gt_boxes = filter_non_gt_boxes
        assert 1 <= len(self.thresholds) <= 4 and 1 <= len(self.topks) <= 4 and max(self.topks) <= 10
        self._n = len(self.thresholds) * len(self.topks) + 1
        self._last = self.prefixes.index("last_") if "last_" in self.prefixes else -1
        self.counters = None
        self.reset()

    # ------------------------------------------------------------------------------------------------ counters
    def _size(self, P):
        return P * 2 * self._n + _N_ANALYSIS

    def _ensure(self, dev):
        if self.counters is None or self.counters.device != dev:
            assert self.counters is None or not bool(self.counters.any()), "counters live on another device"
            self.counters = torch.zeros(self._size(len(self.prefixes)), dtype=torch.int64, device=dev)
        return self.counters

    def reset(self):
        """Zero everything (GroundingEvaluator.reset: same keys, the break-downs' gts start at 1e-14)."""
        base = GroundingEvaluator(self.only_root, self.thresholds, self.topks, self.prefixes, self.filter_non_gt_boxes)
        self._base_dets, self._base_gts = base.dets, base.gts
        if self.counters is not None:
            self.counters.zero_()

    def _totals(self):
        dets, gts = dict(self._base_dets), dict(self._base_gts)
        if self.counters is None:
            return dets, gts
        c = self.counters.cpu().tolist()                       # the one device-to-host copy
        n, nk = self._n, len(self.topks)
        for pi, p in enumerate(self.prefixes):
            for ai, a in enumerate(ALIGNMENTS):
                row = c[(pi * 2 + ai) * n:(pi * 2 + ai + 1) * n]
                for ti, t in enumerate(self.thresholds):
                    for ki, k in enumerate(self.topks):
                        dets[(p, t, k, _MODE[a])] += row[ti * nk + ki]
                        gts[(p, t, k, _MODE[a])] += row[-1]
        an = c[len(self.prefixes) * 2 * n:]
        for ti, suffix in enumerate(("", "50")[:len(self.thresholds)]):
            for fi, (on, off) in enumerate((("vd", "vid"), ("hard", "easy"), ("unique", "multi"))):
                for oi, name in enumerate((on, off)):
                    i = ((ti * 3 + fi) * 2 + oi) * 2
                    dets[name + suffix] += an[i]
                    gts[name + suffix] += an[i + 1]
        return dets, gts

    @property
    def dets(self):
        return self._totals()[0]

    @property
    def gts(self):
        return self._totals()[1]

    def print_stats(self):
        ev = self._as_host_evaluator()
        ev.print_stats()

    def _as_host_evaluator(self):
        ev = GroundingEvaluator(self.only_root, self.thresholds, self.topks, self.prefixes, self.filter_non_gt_boxes)
        ev.dets, ev.gts = self._totals()
        return ev

    def synchronize_between_processes(self):
        """Sum the counters over the ranks (GroundingEvaluator's all-reduce); every rank ends with the totals."""
        ev = self._as_host_evaluator()
        ev.synchronize_between_processes()
        self._base_dets, self._base_gts = ev.dets, ev.gts
        if self.counters is not None:
            self.counters.zero_()

    # ------------------------------------------------------------------------------------------------ evaluation
    def evaluate_all(self, end_points):
        """Every prefix, both alignments: one launch on CUDA tensors.  Reads predictions and targets from end_points, as
        GroundingEvaluator.evaluate does."""
        self._run(end_points, self.prefixes, self._last, None)

    def evaluate(self, end_points, prefix):
        """Drop-in for GroundingEvaluator.evaluate: one prefix, both alignments (one launch + two small adds)."""
        pi = self.prefixes.index(prefix)
        self._run(end_points, [prefix], 0 if prefix == "last_" else -1, pi)

    def _run(self, ep, prefixes, last, into):
        dev = ep[f"{prefixes[0]}center"].device
        main = self._ensure(dev)
        if not prefixes:
            return
        gate = _gate_of(ep, None, self.filter_non_gt_boxes)
        c = main if into is None else torch.zeros(self._size(1), dtype=torch.int64, device=dev)
        if dev.type == "cuda":
            _decode_kernel(ep, ep, prefixes, list(ALIGNMENTS), 10, self.only_root, gate, True, outputs=False, counters=c,
                           thresholds=self.thresholds, topks=self.topks, last_prefix=last)
        else:
            self._count_torch(ep, prefixes, last, gate, c)
        if into is not None:
            n2 = 2 * self._n
            main[into * n2:(into + 1) * n2] += c[:n2]
            main[len(self.prefixes) * n2:] += c[n2:]

    def _count_torch(self, ep, prefixes, last, gate, c):
        out = _decode_torch(ep, ep, prefixes, list(ALIGNMENTS), 10, self.only_root, gate, True)
        iou = out["top_iou"]                                              # (P, 2, B, G, 10)
        B, G = iou.shape[2:4]
        nobj = ep["box_label_mask"].sum(1).long().clamp(max=G)
        valid = torch.arange(G, device=iou.device)[None, :] < nobj[:, None]
        n, nk = self._n, len(self.topks)
        for pi in range(len(prefixes)):
            for ai in range(2):
                base = (pi * 2 + ai) * n
                for ti, t in enumerate(self.thresholds):
                    hit = iou[pi, ai] > t
                    for ki, k in enumerate(self.topks):
                        c[base + ti * nk + ki] += (hit[..., :k].any(-1) & valid).sum()
                c[base + n - 1] += valid.sum()
        if last >= 0 and all(k in ep for k in _FLAGS):
            an = len(prefixes) * 2 * n
            flags = [torch.as_tensor(ep[k]).bool().reshape(B) for k in _FLAGS]
            for ti, t in enumerate(self.thresholds[:2]):
                found = iou[last, 1, :, 0, 0] > t
                for fi, f in enumerate(flags):
                    for oi, sel in enumerate((f, ~f)):
                        i = an + ((ti * 3 + fi) * 2 + oi) * 2
                        c[i] += (found & sel).sum()
                        c[i + 1] += sel.sum()


class PipelinedEvalStep:
    """The forward-only sibling of pipeline.PipelinedTrainStep (same buffers, same rotation), model in eval() under no_grad:

        main   [wait prefetch(i)] point graph(i): rotate, SA/FP stack | rest graph(i): encoder/decoder, heads,
                                                                         evaluate_all / decode into static outputs
        side                      [wait rotation(i)] copy batch i+1, geometry(i+1), text encoder(i+1)

    first_batch: dict of DEVICE tensors, the layout of every later batch; the targets the evaluator / decode read ride
    along as extra keys.  evaluator: a DeviceGroundingEvaluator (its evaluate_all is captured at the end of the rest
    graph: the step then performs no host synchronisation).  decode: None, True or a dict of decode_grounding keywords
    (prefixes, topk, alignment, only_root, filter_non_gt_boxes): its outputs are `self.decoded`, static tensors.
    prefetch: "geometry" (all coordinate-only geometry of the next batch), "sa1" (its SA1 sampling) or None (sampling
    inside the step; the text encoder then runs for the CURRENT batch underneath the point backbone).  after_forward
    (end_points, batch) is captured behind the forward (e.g. a loss for logging).  pre_stage: as in PipelinedTrainStep.
    step(next_batch=...) returns the static end_points (and `decoded`, when asked for) of the batch just run."""

    def __init__(self, model, first_batch, *, evaluator=None, decode=None, prefetch="geometry", text_prefetch=True,
                 stream=None, pre_stage=None, after_forward=None, sa1_samples=2048):
        from . import pointnet2_utils
        prefetch_geometry = prefetch == "geometry"
        text_prefetch = bool(text_prefetch) and prefetch is not None
        self.model, self.evaluator = model, evaluator
        assert not model.training, "PipelinedEvalStep runs the model in eval() mode"
        dev = first_batch["point_clouds"].device
        self.main = stream or torch.cuda.current_stream()
        self.side = _side_stream(dev)
        mode = dict(capture_error_mode="thread_local")
        self.side.wait_stream(self.main)
        with torch.cuda.stream(self.side), torch.no_grad():
            xyz = first_batch["point_clouds"][..., 0:3].contiguous()
            geo_keys, warm = [], []
            if prefetch_geometry:
                geo = model.backbone_net.geometry(xyz)
                geo_keys, warm = list(geo.keys()), list(geo.values())
            elif prefetch is not None:
                warm = [pointnet2_utils.furthest_point_sample(xyz, sa1_samples)]
            text_warm = model.encode_text_frozen(first_batch["tokenized"]["input_ids"], first_batch["tokenized"]["attention_mask"])
        self.side.synchronize()
        flat0 = _flat(first_batch)
        order = flat0 + warm + ([text_warm] if text_prefetch else [])
        self._pack_next, nv = _packed_like(order)
        self._pack_cur, cv = _packed_like(order)
        for v, t in zip(nv, order):
            v.copy_(t)
        self._pack_cur.copy_(self._pack_next)
        nb, ni = len(flat0), len(warm)
        self._nxt_flat, self._cur_flat = nv[:nb], cv[:nb]
        self.nxt, self.cur = _rebuild(first_batch, self._nxt_flat), _rebuild(first_batch, self._cur_flat)
        self.inds_next, self.inds_cur = nv[nb:nb + ni], cv[nb:nb + ni]
        self.text_prefetch = text_prefetch
        self.pre_stage, self.g_pre = pre_stage, None
        if pre_stage is not None:
            pre_stage.bind(inputs={k: self.nxt[k] for k in pre_stage.consumes},
                           outputs={k: self.nxt[k] for k in pre_stage.produces})
            self.g_pre = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.g_pre, stream=self.side, **mode):
                pre_stage()
        tok = (self.nxt if text_prefetch else self.cur)["tokenized"]

        # ---- side stream: geometry / sampling and text encoder of the NEXT batch
        self.g_fps, self.g_text = None, torch.cuda.CUDAGraph()
        if prefetch is not None:
            self.g_fps = torch.cuda.CUDAGraph()
            _lib.check(_lib.lib().eda_fps_set_background(1), "eda_fps_set_background")
            try:
                with torch.cuda.graph(self.g_fps, stream=self.side, **mode), torch.no_grad():
                    xyz_next = self.nxt["point_clouds"][..., 0:3].contiguous()
                    if prefetch_geometry:
                        outs = list(model.backbone_net.geometry(xyz_next).values())
                    else:
                        outs = [pointnet2_utils.furthest_point_sample(xyz_next, sa1_samples)]
                    for v, t in zip(self.inds_next, outs):
                        v.copy_(t)
            finally:
                _lib.check(_lib.lib().eda_fps_set_background(0), "eda_fps_set_background")
        with torch.cuda.graph(self.g_text, stream=self.side, **mode), torch.no_grad():
            hidden = model.encode_text_frozen(tok["input_ids"], tok["attention_mask"])
            if text_prefetch:
                self.text_next = nv[-1]
                self.text_next.copy_(hidden)
            else:
                self.text_next = hidden
        self.side.synchronize()
        if self.g_pre is not None:
            self.g_pre.replay()
        if self.g_fps is not None:
            self.g_fps.replay()
        self.g_text.replay()
        torch.cuda.synchronize()
        self._pack_cur.copy_(self._pack_next)
        self.text_cur = cv[-1] if self.text_prefetch else self.text_next
        inputs_h = dict(self.cur)
        inputs_h["text_hidden"] = self.text_cur
        if prefetch_geometry:
            inputs_h["backbone_geometry"] = dict(zip(geo_keys, self.inds_cur))
        elif prefetch is not None:
            inputs_h["sa1_inds"] = self.inds_cur[0]
        self.inputs = inputs_h

        # ---- main stream: point graph | rest graph
        # one eager forward first: everything the model creates lazily (sampler workspaces of this stream, the decoder's
        # persistent K | V weight stacks, LDS attributes of kernels first used in eval mode) exists before the capture
        with torch.cuda.stream(self.main), torch.no_grad():
            model(first_batch)
        torch.cuda.synchronize()
        if evaluator is not None:
            evaluator._ensure(dev)                             # the counters exist before the capture
        dec_kw = None if not decode else (dict(decode) if isinstance(decode, dict) else {})
        self.decoded = None
        self.g_pts, self.g_rest = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        pool = torch.cuda.graph_pool_handle()
        with torch.cuda.graph(self.g_pts, pool=pool, stream=self.main, **mode), torch.no_grad():
            self._pack_cur.copy_(self._pack_next)              # rotate: one copy of the packed buffer
            ep_static = model.forward_point_backbone(inputs_h)
        with torch.cuda.graph(self.g_rest, pool=pool, stream=self.main, **mode), torch.no_grad():
            ep = model.forward_rest(inputs_h, ep_static)
            view = _EndPointsWithTargets(ep, self.cur)
            if after_forward is not None:
                after_forward(ep, self.cur)
            if evaluator is not None:
                evaluator.evaluate_all(view)
            if dec_kw is not None:
                tg = self.cur if "positive_map" in self.cur else None
                self.decoded = decode_grounding(view, targets=tg, **dec_kw)
        self.end_points = ep
        self.ev_pts, self.ev_fps, self.ev_done, self.ev_text = (torch.cuda.Event() for _ in range(4))
        self.ev_fps.record(self.side)
        self.ev_done.record(self.main)

    def _feed(self, batch):
        if self.pre_stage is not None:
            skip = set(self.pre_stage.produces)
            pairs = []
            for k, dst in self.nxt.items():
                if k in skip and k not in batch:
                    continue
                if k not in batch:
                    raise KeyError(f"next_batch lacks {k!r}")
                pairs += [(dst[kk], batch[k][kk]) for kk in dst] if isinstance(dst, dict) else [(dst, batch[k])]
            pairs = [(v, t) for v, t in pairs if torch.is_tensor(v)]
        else:
            pairs = list(zip(self._nxt_flat, _flat(batch)))
        for v, t in pairs:
            v.copy_(t)
            if t.is_cuda:                   # the copy runs on the side stream: keep the caller's memory alive until it is done
                t.record_stream(self.side)

    def step(self, next_batch=None):
        """Run the batch fed by the previous call (the first batch initially); copy `next_batch` and start its geometry /
        text encoding underneath.  Returns the static end_points, or (end_points, decoded) with decode."""
        caller = torch.cuda.current_stream()
        if caller != self.main:
            self.main.wait_stream(caller)
            with torch.cuda.stream(self.main):
                return self.step(next_batch)
        cur = self.main
        cur.wait_event(self.ev_fps)                # this batch's geometry / hidden states / data are in the nxt buffers
        self.g_pts.replay()
        self.ev_pts.record(cur)
        with torch.cuda.stream(self.side):
            self.side.wait_event(self.ev_pts)      # the rotation has taken its copies: nxt may be overwritten
            if not self.text_prefetch:
                self.side.wait_event(self.ev_done)     # the previous step has consumed the hidden states
                self.g_text.replay()
                self.ev_text.record(self.side)
            if next_batch is not None:
                self._feed(next_batch)
            if self.g_pre is not None:
                self.g_pre.replay()
            if self.g_fps is not None:
                self.g_fps.replay()
            if self.text_prefetch:
                self.g_text.replay()
            self.ev_fps.record(self.side)
        if not self.text_prefetch:
            cur.wait_event(self.ev_text)
        self.g_rest.replay()
        self.ev_done.record(cur)
        return self.end_points if self.decoded is None else (self.end_points, self.decoded)

    def check(self):
        """Host-side health check (synchronises the device): raises if the multi-workgroup sampler ever gave up its spin."""
        n = self.fps_status()
        if n:
            raise RuntimeError(f"furthest point sampling gave up its inter-workgroup spin in {n} workspace(s)")

    def fps_status(self):
        from . import ext
        return ext.fps_status(self.nxt["point_clouds"].device)


class _EndPointsWithTargets:
    """end_points first, the batch's extra keys (targets, detected boxes under the evaluator's names) behind them."""

    _ALIAS = {"all_detected_boxes": "det_boxes", "all_detected_bbox_label_mask": "det_bbox_label_mask"}

    def __init__(self, ep, batch):
        self.ep, self.batch = ep, batch

    def _find(self, k):
        if k in self.ep:
            return self.ep[k]
        if k in self.batch:
            return self.batch[k]
        if k in self._ALIAS and self._ALIAS[k] in self.batch:
            return self.batch[self._ALIAS[k]]
        raise KeyError(k)

    def __getitem__(self, k):
        return self._find(k)

    def __contains__(self, k):
        try:
            self._find(k)
            return True
        except KeyError:
            return False


class SceneHandle:
    """What session.ground() keeps of a scene: the point cloud and the point backbone's end_points (one row)."""

    def __init__(self, point_cloud, end_points):
        self.point_cloud, self.end_points = point_cloud, end_points


class GroundingSession:
    """session.ground(point_cloud, sentences) -> the boxes the sentences refer to, for ONE scene.

    The point backbone (forward_point_backbone) does not depend on the text: it runs once per scene, its end_points are
    expanded (copied, not recomputed) to one row per sentence for forward_rest, and the returned SceneHandle lets a later
    call with other sentences skip it altogether."""

    def __init__(self, model, tokenizer=None):
        self.model = model.eval()
        self.tokenizer = tokenizer if tokenizer is not None else getattr(model, "tokenizer", None)

    def encode_scene(self, point_cloud):
        pc = point_cloud if point_cloud.dim() == 3 else point_cloud[None]
        assert pc.shape[0] == 1, "one scene per call"
        with torch.no_grad():
            ep = self.model.forward_point_backbone({"point_clouds": pc.contiguous()})
        return SceneHandle(pc, ep)

    def ground(self, point_cloud, utterances=None, detected_boxes=None, topk=10, *, tokenized=None, positive_map=None,
               alignment="semantic", prefix="last_", scene=None, explain=False):
        """point_cloud: (N, 3 + C) device tensor (ignored when `scene`, the handle a previous call returned, is given).
        utterances: list of U strings (needs a tokenizer) or a dict {"input_ids", "attention_mask"} of (U, L) tensors;
        `tokenized=` is the same dict by keyword.  detected_boxes: None or (boxes (D, 6), mask (D,), class_ids (D,)) for a
        model with the detected-box stream (None: no detected box, all masked out but the first zero box).
        Token weights of the root object: the caller's positive_map (U, T) or (U, 1, T) if given; else the mask of the
        NON-SPECIAL tokens of each sentence (attention_mask without the first <s> and the last </s> token), every word
        counting alike.  alignment: "semantic" (the reference's `bbf`, the one its `last_` break-downs are taken on) or
        "position".  Returns a dict: boxes (U, topk, 6) centre + size, corners (U, topk, 6), scores (U, topk),
        queries (U, topk), scene (the handle) and end_points.
        explain=True adds "explain": why these boxes -- head-averaged attention maps (eda_amd.attention.record_weights: one
        extra launch per recorded module, every other output bit-identical), with S seed points and L tokens:
        token_to_seeds (U, L, S) the last encoder layer's text <- points map (cross_lv), query_to_tokens (U, topk, L) and
        query_to_seeds (U, topk, S) the rows of the last decoder layer's cross_l / cross_v maps for the returned
        `queries`, seed_xyz (S, 3) and seed_inds (S,) (indices into the point cloud).  upsample_to_points() spreads an
        (..., S) map over the N input points."""
        model = self.model
        if isinstance(utterances, dict) and tokenized is None:
            tokenized, utterances = utterances, None
        if scene is None:
            scene = self.encode_scene(point_cloud)
        dev = scene.point_cloud.device
        if tokenized is None:
            if self.tokenizer is None:
                raise RuntimeError("no tokenizer: pass tokenized={'input_ids', 'attention_mask'}")
            tok = self.tokenizer.batch_encode_plus(list(utterances), padding="longest", return_tensors="pt").to(dev)
            tokenized = {"input_ids": tok["input_ids"], "attention_mask": tok["attention_mask"]}
        ids, am = tokenized["input_ids"].to(dev), tokenized["attention_mask"].to(dev)
        U = ids.shape[0]
        inputs = {"point_clouds": scene.point_cloud.expand(U, -1, -1), "tokenized": {"input_ids": ids, "attention_mask": am}}
        if getattr(model, "butd", False):
            if detected_boxes is None:
                boxes = torch.zeros(132, 6, device=dev)
                mask = torch.zeros(132, dtype=torch.bool, device=dev)
                mask[0] = True                                   # (a fully masked key set has no softmax)
                cls = torch.zeros(132, dtype=torch.long, device=dev)
            else:
                boxes, mask, cls = detected_boxes
            inputs["det_boxes"] = boxes.to(dev)[None].expand(U, -1, -1).contiguous()
            inputs["det_bbox_label_mask"] = mask.to(dev)[None].expand(U, -1).contiguous()
            inputs["det_class_ids"] = cls.to(dev)[None].expand(U, -1).contiguous()
        ep = {k: (v.expand(U, *v.shape[1:]).contiguous() if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == 1 else v)
              for k, v in scene.end_points.items()}
        maps = None
        with torch.no_grad():
            if explain:
                from .attention import record_weights
                sites = (f"cross_encoder.layers.{len(model.cross_encoder.layers) - 1}.cross_layer.cross_lv",
                         f"decoder.{model.num_decoder_layers - 1}.cross_l", f"decoder.{model.num_decoder_layers - 1}.cross_v")
                with record_weights(model, sites) as maps:
                    ep = model.forward_rest(inputs, ep)
            else:
                ep = model.forward_rest(inputs, ep)
            if positive_map is None:
                T = 256
                n_tok = am.sum(1, keepdim=True)
                pos = torch.arange(am.shape[1], device=dev)[None, :]
                w = ((pos >= 1) & (pos < n_tok - 1) & (am > 0)).float()
                positive_map = torch.zeros(U, 1, T, device=dev)
                positive_map[:, 0, :w.shape[1]] = w
            elif positive_map.dim() == 2:
                positive_map = positive_map[:, None, :]
            out = decode_grounding(ep, prefixes=(prefix,), topk=topk, targets={"positive_map": positive_map.to(dev).float()},
                                   only_root=True, alignment=alignment)
        res = {"boxes": out["top_box"][0, 0, :, 0], "corners": out["top_corners"][0, 0, :, 0],
               "scores": out["top_score"][0, 0, :, 0], "queries": out["top_query"][0, 0, :, 0], "scene": scene,
               "end_points": ep}
        if explain:
            lv, cl, cv = (maps[s_] for s_ in sites)
            rows = res["queries"].long()[:, :, None]
            res["explain"] = {"token_to_seeds": lv,
                              "query_to_tokens": torch.gather(cl, 1, rows.expand(-1, -1, cl.shape[2])),
                              "query_to_seeds": torch.gather(cv, 1, rows.expand(-1, -1, cv.shape[2])),
                              "seed_xyz": scene.end_points["fp2_xyz"][0], "seed_inds": scene.end_points["fp2_inds"][0]}
        return res


def upsample_to_points(seed_map, scene):
    """(..., S) values on the seed points of `scene` (a SceneHandle; e.g. a row of explain["query_to_seeds"]) -> (..., N)
    on its input points, for colouring the cloud: the backbone's own feature propagation rule (PointnetFPModule,
    pointnet2/pointnet2_modules.py: three nearest seeds, weights 1 / (distance + 1e-8) normalised) on the existing
    three_nn / three_interpolate kernels.  Every output lies between the minimum and maximum of its map; at a seed point
    itself it is that seed's value."""
    from . import pointnet2_utils
    xyz = scene.point_cloud[..., :3].contiguous().float()                    # (1, N, 3)
    known = scene.end_points["fp2_xyz"].contiguous().float()                  # (1, S, 3)
    S = known.shape[1]
    assert seed_map.shape[-1] == S, f"seed_map must end in the {S} seed points"
    with torch.no_grad():
        dist, idx = pointnet2_utils.three_nn(xyz, known)
        recip = 1.0 / (dist + 1e-8)
        weight = recip / recip.sum(dim=2, keepdim=True)
        feats = seed_map.detach().float().reshape(1, -1, S).contiguous()
        out = pointnet2_utils.three_interpolate(feats, idx, weight)           # (1, C, N)
    return out.reshape(*seed_map.shape[:-1], xyz.shape[1])
