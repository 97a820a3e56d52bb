"""eda_amd.inference on the MI355X: the decode kernel (csrc/ground_decode.hip) against the torch form and the fp64 form,
DeviceGroundingEvaluator against the reference's goldens and against GroundingEvaluator, captured; PipelinedEvalStep
driven like a loader against eager eval forwards; GroundingSession.ground against one ordinary forward."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

import inference_fixtures as IF
import test_inference as TI

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

DEV = "cuda"


def _cases():
    yield from IF.fixture_cases()
    ep, prefixes = IF.bench_case()
    yield "bench_sized", ep, prefixes, False, False


class _CapturingEvaluator:
    """GroundingEvaluator's own fp32 scores on the device: its evaluate_bbox_by_* build the token probabilities, and the
    two einsums of its _accumulate (grounding_evaluator.py:133) are applied to them."""

    def __init__(self, only_root):
        from eda_amd.grounding_evaluator import GroundingEvaluator

        outer = self

        class Ev(GroundingEvaluator):
            def _accumulate(self, ep, prefix, sem, mode):
                pmap = (ep["positive_map"] > 0).to(sem.dtype)
                if self.only_root:
                    pmap = pmap[:, :1]
                extra = (ep["modify_positive_map"][:, 0] + ep["pron_positive_map"][:, 0] + ep["rel_positive_map"][:, 0]
                         - ep["other_entity_map"][:, 0]).to(sem.dtype)
                outer.scores[(prefix, mode)] = (torch.einsum("bqt,bot->boq", sem, pmap)
                                                + torch.einsum("bqt,bt->bq", sem, extra)[:, None, :])
        self.scores = {}
        self.ev = Ev(only_root=only_root, prefixes=[])


def test_kernel_against_torch_form_and_fp64():
    """Indices equal those of the fp64 form except on near-ties (<= 1 % of the slots) and equal the CPU form's on the
    same slots; boxes are copies; IoU to 1e-6; the kernel's score error <= 4 x the evaluator's own fp32 error on this
    device + 1e-6.  Both errors are printed (profiles/inference.md quotes them)."""
    from eda_amd.inference import decode_grounding
    for case, ep, prefixes, only_root, filt in _cases():
        epd = IF.to_device(ep, DEV)
        out = decode_grounding(epd, prefixes=prefixes, topk=10, targets=epd, filter_non_gt_boxes=filt, only_root=only_root)
        torch.cuda.synchronize()
        ref = decode_grounding(ep, prefixes=prefixes, topk=10, targets=ep, filter_non_gt_boxes=filt, only_root=only_root)
        n, left, err_kernel = IF.compare_with_fp64(out, ep, prefixes, only_root, filt)
        # against the CPU form: same indices wherever the fp64 form has no near-tie, boxes of equal indices bit-equal
        same = out["top_query"].cpu() == ref["top_query"]
        assert float((~same).sum()) <= IF.MAX_LEFT_OUT * same.numel(), case
        assert torch.equal(out["top_box"].cpu()[same], ref["top_box"][same])
        assert torch.equal(out["top_corners"].cpu()[same], ref["top_corners"][same])
        assert float((out["top_iou"].cpu()[same] - ref["top_iou"][same]).abs().max()) <= 1e-6
        # the path it replaces, in its own arithmetic on this device, against the same fp64 form
        cap = _CapturingEvaluator(only_root)
        err_torch = 0.0
        for p in prefixes:
            cap.ev.evaluate(epd, p)
            for a, mode in (("position", "bbs"), ("semantic", "bbf")):
                want = IF.fp64_scores(ep, p, a, only_root)          # (ungated on both sides: the gate only zeroes)
                err_torch = max(err_torch, float((cap.scores[(p, mode)].double().cpu() - want).abs().max()))
        print(f"{case}: {n} slots, {left} near-ties left out; largest score error: kernel {err_kernel:.3e}, "
              f"GroundingEvaluator fp32 on this device {err_torch:.3e}")
        assert err_kernel <= 4 * err_torch + 1e-6, (case, err_kernel, err_torch)


def test_tie_rule_lowest_query_first_gpu():
    TI.check_tie_rule(DEV)


def test_device_evaluator_counters_equal_the_reference_gpu():
    TI.check_golden_counters(DEV)
    TI.check_golden_counters(DEV, how="each")


def _evaluators(prefixes, only_root=False):
    from eda_amd.grounding_evaluator import GroundingEvaluator
    from eda_amd.inference import DeviceGroundingEvaluator
    kw = dict(only_root=only_root, thresholds=[0.25, 0.5], topks=[1, 5, 10], prefixes=prefixes)
    return GroundingEvaluator(**kw), DeviceGroundingEvaluator(**kw)


def test_device_evaluator_equals_grounding_evaluator_bench_sized():
    ep, prefixes = IF.bench_case()
    epd = IF.to_device(ep, DEV)
    for only_root in (False, True):
        host, devev = _evaluators(prefixes, only_root)
        for p in prefixes:
            host.evaluate(epd, p)
        devev.evaluate_all(epd)
        d, g = devev.dets, devev.gts
        assert set(d) == set(host.dets)
        bad = [(k, d[k], host.dets[k]) for k in host.dets if d[k] != host.dets[k]]
        assert not bad, bad[:8]
        assert all(abs(g[k] - host.gts[k]) <= 1e-12 for k in host.gts)
        assert sum(d.values()) > 0 and any(d[k] < g[k] - 0.5 for k in d)


def test_evaluate_all_captured_and_replayed():
    ep, prefixes = IF.bench_case()
    epd = IF.to_device(ep, DEV)
    _, once = _evaluators(prefixes)
    once.evaluate_all(epd)
    want = once.dets, once.gts
    _, ev = _evaluators(prefixes)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ev.evaluate_all(epd)                      # warm-up: counters allocated, LDS attribute set
        torch.cuda.synchronize()
        ev.reset()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            ev.evaluate_all(epd)
        torch.cuda.synchronize()
        assert sum(ev.dets.values()) == 0, "a capture must not run the kernel"
        for _ in range(3):
            g.replay()
        torch.cuda.synchronize()
    torch.cuda.current_stream().wait_stream(s)
    d, t = ev.dets, ev.gts
    assert all(d[k] == 3 * want[0][k] for k in d), [(k, d[k], want[0][k]) for k in d if d[k] != 3 * want[0][k]][:5]
    for k in t:
        base = 1e-14 if isinstance(k, str) else 0
        assert abs((t[k] - base) - 3 * (want[1][k] - base)) <= 1e-9, k


def test_evaluate_all_does_not_synchronise():
    ep, prefixes = IF.bench_case()
    epd = IF.to_device(ep, DEV)
    _, ev = _evaluators(prefixes)
    ev.evaluate_all(epd)
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("error")
    except Exception as e:                        # noqa: BLE001
        pytest.skip(f"torch.cuda.set_sync_debug_mode is not supported by this torch build on ROCm: {e}")
    try:
        ev.evaluate_all(epd)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert ev.gts[(prefixes[0], 0.25, 1, "bbs")] == 2 * int(ep["box_label_mask"].sum())


# ------------------------------------------------------------------------------------------- the pipelined eval step
MODEL_PREFIXES = ["proposal_", "0head_", "last_"]          # num_decoder_layers = 2


def _eval_batch(seed, scenes, dev, points, tokens):
    """bench.make_inputs + the synthetic grounding targets and the analysis flags, all on the device."""
    import bench
    from eda_amd import synthetic
    batch = bench.make_inputs(seed, scenes, dev, points, tokens)
    tg = synthetic.grounding_targets(seed, scenes, batch["point_clouds"][..., :3].cpu().numpy(),
                                     batch["tokenized"]["attention_mask"].cpu().numpy())
    for k, v in tg.items():
        batch[k] = torch.from_numpy(v).to(dev)
    rng = np.random.default_rng(500 + seed)
    for k in ("is_view_dep", "is_hard", "is_unique"):
        batch[k] = torch.from_numpy(rng.integers(0, 2, scenes).astype(bool)).to(dev)
    return batch


def _positive_sizes(model):
    """A freshly initialised size head predicts negative sizes, which GroundingEvaluator refuses (as the reference does,
    src/grounding_evaluator.py:170): shift every size head as a trained model's is, towards sizes around 0.8."""
    with torch.no_grad():
        for name, m in model.named_modules():
            if name.endswith("size_pred_head"):
                m.net[8].weight.mul_(0.1)
                m.net[8].bias.fill_(0.8)
    return model


def _tensor_items(ep):
    return {k: v for k, v in ep.items() if torch.is_tensor(v)}


@pytest.mark.parametrize("prefetch", ["geometry", "sa1", None])
def test_pipelined_eval_step_with_rotating_batches(prefetch):
    """Three different batches in rotation, 6 steps: per step `cur` holds the batch being run, the sampling indices are
    the FPS of that batch, and every tensor of the step's end_points is BIT-equal to an eager model.eval() forward of an
    identical model on that batch; the device counters after the 6 steps equal GroundingEvaluator's on the eager
    end_points."""
    import check_graph_vs_eager as C
    from eda_amd import pointnet2_utils
    from eda_amd.grounding_evaluator import GroundingEvaluator
    from eda_amd.inference import DeviceGroundingEvaluator, PipelinedEvalStep
    dev = torch.device("cuda", 0)
    scenes, points, tokens, steps = 2, 20000, 24, 6
    a = _positive_sizes(C.make(0, dev, num_queries=64, num_decoder_layers=2).eval())
    b = copy.deepcopy(a).to(dev)       # (MultiheadAttention.__deepcopy__ builds its copy on the host)
    batches = [_eval_batch(s, scenes, dev, points, tokens) for s in (0, 5, 9)]
    assert not torch.equal(batches[0]["point_clouds"], batches[1]["point_clouds"])
    seq = [batches[i % 3] for i in range(steps + 1)]
    kw = dict(only_root=True, thresholds=[0.25, 0.5], topks=[1, 5, 10], prefixes=MODEL_PREFIXES)
    host, devev = GroundingEvaluator(**kw), DeviceGroundingEvaluator(**kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        eager = []
        for i in range(steps):
            ep = a(seq[i])
            for p in MODEL_PREFIXES:
                host.evaluate({**ep, **seq[i]}, p)
            eager.append({k: v.clone() for k, v in _tensor_items(ep).items()})
        torch.cuda.synchronize()
        pipe = PipelinedEvalStep(b, seq[0], evaluator=devev, decode=dict(prefixes=MODEL_PREFIXES, only_root=True),
                                 prefetch=prefetch, stream=side)
        for i in range(steps):
            ep, decoded = pipe.step(next_batch=seq[i + 1])
            torch.cuda.synchronize()
            assert torch.equal(pipe.cur["point_clouds"], seq[i]["point_clouds"]), f"step {i}: wrong points"
            assert torch.equal(pipe.cur["tokenized"]["input_ids"], seq[i]["tokenized"]["input_ids"]), f"step {i}: wrong tokens"
            assert torch.equal(pipe.cur["positive_map"], seq[i]["positive_map"]), f"step {i}: wrong targets"
            if prefetch is not None:
                want = pointnet2_utils.furthest_point_sample(seq[i]["point_clouds"][..., 0:3].contiguous(), 2048)
                assert torch.equal(pipe.inds_cur[0], want), f"step {i}: the indices used are not the FPS of the batch run"
            tok = seq[i]["tokenized"]
            hidden = b.encode_text_frozen(tok["input_ids"], tok["attention_mask"])
            torch.testing.assert_close(pipe.text_cur, hidden, rtol=1e-5, atol=1e-5)      # (tests/test_pipeline_gpu.py's check)
            got = _tensor_items(ep)
            assert set(eager[i]) <= set(got), set(eager[i]) - set(got)
            diff = {k: float((got[k].double() - v.double()).abs().max()) for k, v in eager[i].items()
                    if not torch.equal(got[k], v)}
            assert not diff, (f"step {i}: not bit-equal to the eager forward", diff)
            # the decode captured in the rest graph saw this batch's outputs and targets
            top1 = decoded["top_query"][MODEL_PREFIXES.index("last_"), 1, :, 0, 0]
            ref = pipe_decode_reference(eager[i], seq[i])
            assert torch.equal(top1, ref), f"step {i}: decode of another batch"
            torch.cuda.synchronize()
            if prefetch is not None:
                nxt = pointnet2_utils.furthest_point_sample(seq[i + 1]["point_clouds"][..., 0:3].contiguous(), 2048)
                assert torch.equal(pipe.inds_next[0], nxt), f"step {i}: prefetch of the wrong batch"
        assert pipe.fps_status() == 0
        pipe.check()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    d, g = devev.dets, devev.gts
    bad = [(k, d[k], host.dets[k]) for k in host.dets if d[k] != host.dets[k]]
    assert not bad, bad[:8]
    assert all(abs(g[k] - host.gts[k]) <= 1e-12 for k in host.gts)
    assert g[("last_", 0.25, 1, "bbf")] == steps * scenes
    # three different batches give different outputs: a hand-over that is off by one batch cannot pass the bit comparison
    assert not torch.equal(eager[0]["last_center"], eager[1]["last_center"])


def pipe_decode_reference(ep, batch):
    from eda_amd.inference import decode_grounding
    out = decode_grounding({**ep, **batch}, prefixes=["last_"], targets=batch, only_root=True, alignment="semantic")
    return out["top_query"][0, 0, :, 0, 0]


# ------------------------------------------------------------------------------------------------ the session
def test_grounding_session_one_scene_five_sentences():
    """ground() for one scene and 5 sentences against ONE ordinary eval forward of the scene repeated 5 times with the
    same SA1 indices: top-1 query (index rule of the decode tests), box and score agree within the full-model tolerance
    (rtol 1e-4, atol 1e-5 x max: the row count changes which GEMM variant the backbone runs); the point backbone runs
    once, and not at all when the scene handle is passed back."""
    import bench
    import check_graph_vs_eager as C
    from eda_amd import pointnet2_utils
    from eda_amd.inference import GroundingSession, decode_grounding
    dev = torch.device("cuda", 0)
    U, points, tokens = 5, 20000, 24
    model = C.make(0, dev, num_queries=64, num_decoder_layers=2).eval()
    inputs = bench.make_inputs(3, U, dev, points, tokens)
    scene = inputs["point_clouds"][0]
    tok = inputs["tokenized"]
    det = (inputs["det_boxes"][0], inputs["det_bbox_label_mask"][0], inputs["det_class_ids"][0])
    calls = []
    inner = model.forward_point_backbone
    model.forward_point_backbone = lambda x: (calls.append(1), inner(x))[1]
    session = GroundingSession(model)
    with torch.no_grad():
        res = session.ground(scene, tok, detected_boxes=det, topk=10)
        torch.cuda.synchronize()
        assert len(calls) == 1
        assert res["boxes"].shape == (U, 10, 6) and res["scores"].shape == (U, 10) and res["queries"].shape == (U, 10)
        # the ordinary forward of the repeated scene
        rep = dict(inputs)
        rep["point_clouds"] = scene[None].expand(U, -1, -1).contiguous()
        rep["det_boxes"], rep["det_bbox_label_mask"], rep["det_class_ids"] = (t[None].expand(U, *t.shape).contiguous() for t in det)
        inds = pointnet2_utils.furthest_point_sample(scene[None, :, 0:3].contiguous(), 2048)
        rep["sa1_inds"] = inds.expand(U, -1).contiguous()
        del model.forward_point_backbone
        ep = model(rep)
        am = tok["attention_mask"]
        n_tok = am.sum(1, keepdim=True)
        pos = torch.arange(am.shape[1], device=dev)[None, :]
        pmap = torch.zeros(U, 1, 256, device=dev)
        pmap[:, 0, :am.shape[1]] = ((pos >= 1) & (pos < n_tok - 1) & (am > 0)).float()
        want = decode_grounding(ep, prefixes=["last_"], targets={"positive_map": pmap}, only_root=True, alignment="semantic")
        torch.cuda.synchronize()

        def close(x, y, name):
            tol = 1e-4 * y.abs() + 1e-5 * float(y.abs().max())
            assert bool(((x - y).abs() <= tol).all()), (name, float((x - y).abs().max()), float(y.abs().max()))
        for k in ("last_center", "last_pred_size", "last_sem_cls_scores", "last_proj_queries", "proj_tokens"):
            close(res["end_points"][k], ep[k], k)
        # top-1 per sentence: same query unless the fp64 scores of the two leading queries are a near-tie
        ep_cpu = {k: v.cpu() for k, v in ep.items() if torch.is_tensor(v)}
        ep_cpu["positive_map"] = pmap.cpu()
        for k in IF.AUX:
            ep_cpu[k] = torch.zeros(U, 1, 256)
        _, top, ranked = IF.fp64_decode(ep_cpu, "last_", "semantic", True)
        q_got, q_want = res["queries"][:, 0].cpu(), want["top_query"][0, 0, :, 0, 0].cpu()
        for u in range(U):
            gap = float(ranked[u, 0, 0] - ranked[u, 0, 1])
            print(f"sentence {u}: top-1 query {int(q_got[u])} / {int(q_want[u])}, fp64 gap to the second {gap:.3e}")
            assert int(q_want[u]) == int(top[u, 0, 0]) or gap < IF.TIE
            assert int(q_got[u]) == int(q_want[u]) or gap < IF.TIE, u
            if int(q_got[u]) == int(q_want[u]):
                close(res["boxes"][u, 0], want["top_box"][0, 0, u, 0, 0], "box")
                close(res["scores"][u, :1], want["top_score"][0, 0, u, 0, :1], "score")
        # other sentences on the same scene: the handle is reused, the backbone does not run again
        model.forward_point_backbone = lambda x: (calls.append(1), inner(x))[1]
        tok2 = bench.make_inputs(4, U, dev, points, tokens)["tokenized"]
        res2 = session.ground(None, tokenized=tok2, detected_boxes=det, scene=res["scene"], alignment="position")
        torch.cuda.synchronize()
        assert len(calls) == 1 and res2["boxes"].shape == (U, 10, 6)
        assert not torch.equal(res2["scores"], res["scores"])
        del model.forward_point_backbone
