"""Detection mAP at ScanNet-val size (312 scenes x 256 queries x 18 classes, IoU thresholds 0.25 and 0.5): the device
path of eda_amd/ap_helper.py against its CPU form on the same input.  Prints one JSON line:
    parse_nms_us_per_batch   parse_predictions(as_tensors=True) + parse_groundtruths of one 8-scene batch (median, us)
    nms_device_us_per_batch  the NMS launch of one batch alone, between events (median, us)
    compute_metrics_ms       compute_metrics_at((0.25, 0.5)) over the 312 accumulated scenes, copy included (median, ms)
    cpu_parse_s / cpu_metrics_s / cpu_total_s   the CPU form (tuple lists, numpy) on the same input
    python tools/bench_det_eval.py [--scenes 312] [--reps 5]
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import det_eval_fixtures as DF  # noqa: E402
from eda_amd import ap_helper as AH  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=312)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    cfg = dict(DF.config("eda"), dataset_config=types.SimpleNamespace(num_class=DF.NUM_CLASS))
    ep = DF.make_end_points(11, args.scenes, 256, 132, objectness=False)
    batches = [{k: torch.from_numpy(v[b:b + args.batch].copy()) for k, v in ep.items()}
               for b in range(0, args.scenes, args.batch)]
    out = {"scenes": args.scenes, "queries": 256, "classes": DF.NUM_CLASS, "thresholds": list(DF.THRESHOLDS)}
    if torch.cuda.is_available():
        dev = torch.device("cuda", 0)
        gb = [{k: v.to(dev) for k, v in b.items()} for b in batches]
        torch.cuda.synchronize()
        calc = AH.APCalculator(0.25)
        for rep in range(args.reps + 1):                           # the first pass warms up
            calc.reset()
            times = []
            for b in gb:
                t0 = time.perf_counter()
                rec = (AH.parse_predictions(b, cfg, DF.PREFIX, True, as_tensors=True),
                       AH.parse_groundtruths(b, cfg, True, as_tensors=True))
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
                calc.step(*rec)
        out["parse_nms_us_per_batch"] = round(float(np.median(times)) * 1e6, 1)
        # the NMS launch alone on one batch's decoded boxes (device time between events)
        r = rec[0]
        cls = r.sem_cls
        p = AH.parse_predictions(gb[0], dict(cfg, per_class_proposal=False), DF.PREFIX, True, as_tensors=True)
        score = p.conf[..., 0].double()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        nt = []
        for _ in range(args.reps + 1):
            ev[0].record()
            AH.nms_3d(r.aabb, score, cls, cfg["nms_iou"], cfg["use_old_type_nms"], cfg["cls_nms"])
            ev[1].record()
            torch.cuda.synchronize()
            nt.append(ev[0].elapsed_time(ev[1]) * 1e3)
        out["nms_device_us_per_batch"] = round(float(np.median(nt[1:])), 1)
        mt = []
        for rep in range(args.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = calc.compute_metrics_at(DF.THRESHOLDS)
            mt.append(time.perf_counter() - t0)
        out["compute_metrics_ms"] = round(float(np.median(mt[1:])) * 1e3, 2)
        out["gpu_mAP"] = [round(r["mAP"], 6) for r in res]
        out["device"] = torch.cuda.get_device_name(0)
    if not args.no_cpu:
        t0 = time.perf_counter()
        calc = AH.APCalculator(0.25)
        for b in batches:
            calc.step(AH.parse_predictions(b, cfg, DF.PREFIX, True), AH.parse_groundtruths(b, cfg, True))
        t1 = time.perf_counter()
        res_c = calc.compute_metrics_at(DF.THRESHOLDS)
        t2 = time.perf_counter()
        out["cpu_parse_s"] = round(t1 - t0, 3)
        out["cpu_metrics_s"] = round(t2 - t1, 3)
        out["cpu_total_s"] = round(t2 - t0, 3)
        out["cpu_mAP"] = [round(r["mAP"], 6) for r in res_c]
        if "compute_metrics_ms" in out:
            gpu_total = out["parse_nms_us_per_batch"] * 1e-6 * len(batches) + out["compute_metrics_ms"] * 1e-3
            out["speedup_total"] = round(out["cpu_total_s"] / gpu_total, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
