"""Inference timings at the bench workload (8 x 50 000 points, 256 queries, 80 tokens, 6 decoder layers, fp32):

  (a) eager model.eval() forward + GroundingEvaluator.evaluate over the 7 prefixes   -- the path without eda_amd.inference
  (b) PipelinedEvalStep with DeviceGroundingEvaluator (two graphs + side stream, counters on the device)
  (c) the decode launch alone (DeviceGroundingEvaluator.evaluate_all, eager and as a graph replay) against the 14
      _accumulate chains of GroundingEvaluator on the same end_points
  (d) GroundingSession.ground for ONE scene and U = 1, 8, 32 sentences against U single-sentence forwards, and the share
      of a single forward that the point backbone is
  (e) --forward-only N: N eager eval forwards and nothing else, to be run under rocprofv3 --kernel-trace --stats

Every figure: `--repeats` measurements of `--steps` iterations each, timed with events around the whole loop (one
synchronisation per measurement); reported as median and spread (max - min) in ms per iteration.  One JSON line.
A freshly initialised size head predicts negative sizes, which GroundingEvaluator refuses (as the reference does); the
size heads are shifted to positive sizes, which changes no kernel's work."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")


def measure(fn, steps, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / steps)
    return {"median_ms": round(statistics.median(out), 4), "spread_ms": round(max(out) - min(out), 4),
            "runs_ms": [round(x, 4) for x in out]}


def make_batch(seed, scenes, dev, points, tokens):
    import bench
    import numpy as np
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--points", type=int, default=50000)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--tokens", type=int, default=80)
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sentences", type=int, nargs="*", default=[1, 8, 32])
    ap.add_argument("--forward-only", type=int, default=0, metavar="N")
    ap.add_argument("--skip", default="", help="comma list of parts to leave out: a,b,c,d")
    args = ap.parse_args()
    import bench
    from eda_amd.bdetr import BeaUTyDETR
    from eda_amd.grounding_evaluator import GroundingEvaluator
    from eda_amd.inference import DeviceGroundingEvaluator, GroundingSession, PipelinedEvalStep
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = BeaUTyDETR(num_queries=args.queries, num_decoder_layers=args.layers).to(dev).eval()
    with torch.no_grad():
        for name, m in model.named_modules():
            if name.endswith("size_pred_head"):
                m.net[8].weight.mul_(0.1)
                m.net[8].bias.fill_(0.8)
    prefixes = ["proposal_"] + [f"{i}head_" for i in range(args.layers - 1)] + ["last_"]
    batches = [make_batch(s, args.scenes, dev, args.points, args.tokens) for s in (0, 1, 2)]
    skip = set(args.skip.split(","))
    out = {"workload": vars(args), "prefixes": prefixes}
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream), torch.no_grad():
        if args.forward_only:
            for i in range(args.forward_only + 2):
                model(batches[i % 3])
            torch.cuda.synchronize()
            print(json.dumps({"forward_only": args.forward_only}))
            return
        kw = dict(only_root=True, thresholds=[0.25, 0.5], topks=[1, 5, 10], prefixes=prefixes)
        host, devev = GroundingEvaluator(**kw), DeviceGroundingEvaluator(**kw)
        it = {"i": 0}

        def eager_step():
            b = batches[it["i"] % 3]
            it["i"] += 1
            ep = model(b)
            view = {**ep, **b}
            for p in prefixes:
                host.evaluate(view, p)
        if "a" not in skip:
            out["a_eager_forward_plus_evaluator"] = measure(eager_step, args.steps, args.repeats)
        if "b" not in skip:
            pipe = PipelinedEvalStep(model, batches[0], evaluator=devev, prefetch="geometry", stream=stream)
            jt = {"i": 1}

            def pipe_step():
                pipe.step(next_batch=batches[jt["i"] % 3])
                jt["i"] += 1
            out["b_pipelined_eval_step"] = measure(pipe_step, args.steps, args.repeats)
            pipe.check()
            if "a" not in skip:
                a, b = out["a_eager_forward_plus_evaluator"], out["b_pipelined_eval_step"]
                out["b_scenes_per_s"] = round(args.scenes / b["median_ms"] * 1e3, 2)
                out["a_scenes_per_s"] = round(args.scenes / a["median_ms"] * 1e3, 2)
                out["b_beats_a_by_more_than_the_spreads"] = bool(a["median_ms"] - b["median_ms"] > a["spread_ms"] + b["spread_ms"])
        if "c" not in skip:
            ep = model(batches[0])
            view = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in {**ep, **batches[0]}.items()}
            torch.cuda.synchronize()
            ev_c = DeviceGroundingEvaluator(**kw)
            out["c_decode_launch_eager"] = measure(lambda: ev_c.evaluate_all(view), 50, args.repeats)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=stream):
                ev_c.evaluate_all(view)
            out["c_decode_launch_graph_replay"] = measure(g.replay, 50, args.repeats)

            def chains():
                for p in prefixes:
                    host.evaluate(view, p)
            out["c_fourteen_accumulate_chains"] = measure(chains, 10, args.repeats)
        if "d" not in skip:
            session = GroundingSession(model)
            scene = batches[0]["point_clouds"][0]
            det = (batches[0]["det_boxes"][0], batches[0]["det_bbox_label_mask"][0], batches[0]["det_class_ids"][0])
            one = {k: (v[:1] if torch.is_tensor(v) else {kk: vv[:1] for kk, vv in v.items()})
                   for k, v in bench.make_inputs(0, 1, dev, args.points, args.tokens).items()}
            out["d_single_forward_one_sentence"] = measure(lambda: model(one), 5, args.repeats)
            out["d_point_backbone_one_scene"] = measure(lambda: model.forward_point_backbone(one), 5, args.repeats)
            out["d_backbone_share_of_a_single_forward"] = round(
                out["d_point_backbone_one_scene"]["median_ms"] / out["d_single_forward_one_sentence"]["median_ms"], 3)
            for U in args.sentences:
                tok = bench.make_inputs(7, U, dev, 1000, args.tokens)["tokenized"]
                out[f"d_ground_U{U}"] = measure(lambda: session.ground(scene, tok, detected_boxes=det), 3, args.repeats, warmup=1)
                out[f"d_U{U}_single_forwards_ms"] = round(U * out["d_single_forward_one_sentence"]["median_ms"], 3)
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
