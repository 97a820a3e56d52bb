"""Shared by tests/test_inference.py and tests/test_inference_gpu.py: the fp64 form of the grounding decode that both the
CPU form and the kernel are judged against, the slot-comparison rule, and a bench-sized seeded case."""
import numpy as np
import torch

import eval_fixtures as EF

AUX = ("modify_positive_map", "pron_positive_map", "rel_positive_map", "other_entity_map")
TIE = 1e-6           # a slot is left out of the index comparison only if its fp64 score is this close to a neighbour's
MAX_LEFT_OUT = 0.01  # ... and at most this share of the slots


def fp64_scores(ep, prefix, alignment, only_root, gate=None):
    """(B, G, Q) float64 scores: softmax, token products and sums all in fp64 from the fp32 inputs."""
    if alignment == "position":
        sm = ep[f"{prefix}sem_cls_scores"].double().softmax(-1)
    else:
        sim = torch.matmul(ep[f"{prefix}proj_queries"].double(), ep["proj_tokens"].double().transpose(-1, -2))
        sm = (sim / 0.07).softmax(-1)
    T = ep["positive_map"].shape[-1]
    sem = sm.new_zeros(sm.shape[0], sm.shape[1], T)
    sem[:, :, :sm.shape[-1]] = sm
    pmap = (ep["positive_map"] > 0).double()
    if only_root:
        pmap = pmap[:, :1]
    extra = (ep[AUX[0]][:, 0].double() + ep[AUX[1]][:, 0].double() + ep[AUX[2]][:, 0].double() - ep[AUX[3]][:, 0].double())
    scores = torch.einsum("bqt,bot->boq", sem, pmap) + torch.einsum("bqt,bt->bq", sem, extra)[:, None, :]
    if gate is not None:
        scores = scores * gate.double()[:, None, :]
    return scores


def fp64_decode(ep, prefix, alignment, only_root, gate=None, K=10):
    """scores (B, G, Q) fp64, their stable descending ranking top (B, G, K + 1) and the ranked scores (B, G, K + 1)."""
    scores = fp64_scores(ep, prefix, alignment, only_root, gate)
    s, top = torch.sort(scores, dim=-1, descending=True, stable=True)
    return scores, top[..., :K + 1], s[..., :K + 1]


def comparable_slots(ranked, K=10):
    """(B, G, K) bool: slots whose fp64 score is further than TIE from the previous and the next rank's.  EXACTLY equal
    scores (queries the detected-box gate zeroed, identical rows) are not near-ties: the tie rule decides them, in any
    precision, so they are compared."""
    gap = (ranked[..., :-1] - ranked[..., 1:]).abs()                  # (B, G, K): gap[r] between rank r and r + 1
    far = (gap >= TIE) | (gap == 0)
    ok = far[..., :K].clone()
    ok[..., 1:] &= far[..., :K - 1]
    return ok


def boxes_of(ep, prefix, top):
    """fp32 centre + size boxes and their IoU with each object's ground truth, for the queries `top` (B, G, K)."""
    from eda_amd.grounding_evaluator import _iou3d_pairs
    from eda_amd.losses import box_cxcyczwhd_to_xyzxyz
    pred = torch.cat([ep[f"{prefix}center"], ep[f"{prefix}pred_size"]], -1)
    B, G, K = top.shape
    box = torch.gather(pred[:, None].expand(B, G, pred.shape[1], 6), 2, top[..., None].expand(B, G, K, 6))
    gt = torch.cat([ep["center_label"][:, :G, 0:3], ep["size_gts"][:, :G]], -1)
    iou = _iou3d_pairs(box_cxcyczwhd_to_xyzxyz(gt)[:, :, None, :], box_cxcyczwhd_to_xyzxyz(box))
    return box, iou


def bench_case(seed=7, B=8, Q=256, L=80, T=256, G=132, P=7):
    """A bench-sized batch of outputs and targets: 8 scenes, 256 queries, 256 token slots, 7 heads, 1..132 annotated
    objects per scene (scene 0 has all 132); some queries sit near annotated boxes and lean towards their tokens, so the
    counters have hits and misses at every threshold and k."""
    rng = np.random.default_rng(seed)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))            # noqa: E731
    u = lambda lo, hi, *s: torch.from_numpy(rng.uniform(lo, hi, s).astype(np.float32))     # noqa: E731
    prefixes = ["proposal_", "last_"] + [f"{i}head_" for i in range(P - 2)]
    ep = {}
    pt = f(B, L, 64)
    ep["proj_tokens"] = pt / pt.norm(dim=-1, keepdim=True)
    nobj = rng.integers(1, G + 1, B)
    nobj[0], nobj[1] = G, 1
    mask = torch.zeros(B, G)
    for b in range(B):
        mask[b, :nobj[b]] = 1
    ep["box_label_mask"] = mask
    ep["center_label"] = u(-3, 3, B, G, 3)
    ep["size_gts"] = u(0.2, 1.5, B, G, 3)

    def token_map(p_on):
        m = (rng.uniform(0, 1, (B, G, T)) < p_on).astype(np.float32)
        m[:, :, L:] = 0
        s = m.sum(-1, keepdims=True)
        return torch.from_numpy(np.where(s > 0, m / np.maximum(s, 1), 0).astype(np.float32))
    ep["positive_map"] = token_map(0.04)
    for b in range(B):
        for g in range(G):
            if ep["positive_map"][b, g].sum() == 0:
                ep["positive_map"][b, g, 1 + g % (L - 2)] = 1.0
    for k, p_on in zip(AUX, (0.05, 0.03, 0.04, 0.04)):
        ep[k] = token_map(p_on)
    for p in prefixes:
        ep[f"{p}center"] = u(-3, 3, B, Q, 3)
        ep[f"{p}pred_size"] = u(0.2, 1.5, B, Q, 3)
        ep[f"{p}sem_cls_scores"] = f(B, Q, T)
        pq = f(B, Q, 64)
        for b in range(B):
            for o in rng.choice(int(nobj[b]), min(int(nobj[b]), 24), replace=False):
                for q in rng.choice(Q, 3, replace=False):
                    ep[f"{p}center"][b, q] = ep["center_label"][b, o] + torch.from_numpy(rng.normal(0, 0.2, 3).astype(np.float32))
                    ep[f"{p}pred_size"][b, q] = ep["size_gts"][b, o] * float(rng.uniform(0.7, 1.4))
                    tok = (ep["positive_map"][b, o] > 0).float()
                    ep[f"{p}sem_cls_scores"][b, q] += float(rng.uniform(0.5, 3.0)) * tok
                    pq[b, q] += float(rng.uniform(0.2, 1.0)) * (tok[:L, None] * ep["proj_tokens"][b]).sum(0)
        ep[f"{p}proj_queries"] = pq / pq.norm(dim=-1, keepdim=True)
    for k in ("is_view_dep", "is_hard", "is_unique"):
        ep[k] = torch.from_numpy(rng.integers(0, 2, B).astype(bool))
    return ep, prefixes


def to_device(ep, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in ep.items()}


def fixture_cases():
    """(name, end_points, prefixes, only_root, filter) of the three evaluator fixtures."""
    for case, (seed, only_root, filt) in EF.CASES.items():
        yield case, EF.make_end_points(seed), list(EF.PREFIXES), only_root, filt


def compare_with_fp64(out, ep, prefixes, only_root, filt, box_exact=True, iou_atol=1e-6):
    """Judge decode outputs `out` (tensors (P, 2, B, G, 10[, 6]), any device) against the fp64 form built from the CPU
    end_points `ep`: indices equal on every comparable slot, boxes of equal indices equal (copies), IoUs to iou_atol.
    Returns (slots, left out, largest |top_score - fp64 score of the same query|)."""
    from eda_amd import inference
    out = {k: v.cpu() for k, v in out.items()}
    slots = left_out = 0
    score_err = 0.0
    for pi, p in enumerate(prefixes):
        gate = None
        if filt:
            gate = inference.detected_box_gate(ep, p, ep["all_detected_boxes"], ep["all_detected_bbox_label_mask"])
        for ai, a in enumerate(inference.ALIGNMENTS):
            scores, top, ranked = fp64_decode(ep, p, a, only_root, gate)
            ok = comparable_slots(ranked)
            got = out["top_query"][pi, ai].long()
            same = got == top[..., :10]
            assert bool((same | ~ok).all()), (p, a, "indices differ on slots that are not near-ties")
            slots += ok.numel()
            left_out += int((~ok).sum())
            box, iou = boxes_of(ep, p, got)
            if box_exact:
                assert torch.equal(out["top_box"][pi, ai], box), (p, a, "boxes are not copies")
            else:
                torch.testing.assert_close(out["top_box"][pi, ai], box, rtol=0, atol=0)
            assert float((out["top_iou"][pi, ai] - iou).abs().max()) <= iou_atol, (p, a, "IoU")
            want = torch.gather(scores, 2, got)
            score_err = max(score_err, float((out["top_score"][pi, ai].double() - want).abs().max()))
    assert left_out <= MAX_LEFT_OUT * slots, (left_out, slots)
    return slots, left_out, score_err
