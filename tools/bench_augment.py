"""Device augmentation (eda_amd/augment.py, csrc/augment.hip) at the bench shapes.  Prints one JSON line:
    eager_us_per_batch     AugmentStage() launched eagerly, between device events (median over reps)
    graph_us_per_batch     the same stage captured once and replayed (median)
    launches               kernel launches per batch
    pipe_ms_no_stage / pipe_ms_with_stage   PipelinedTrainStep (8 x 50 000 points, synthetic loss, clipped SGD) per
                           step without and with the stage as its pre_stage (median of --steps steps)
    cpu_ms_per_scene       the CPU form (numpy) per scene on one thread
    python tools/bench_augment.py [--scenes 8] [--points 50000] [--reps 200] [--steps 30] [--no-pipe]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from eda_amd import augment as A  # noqa: E402


def make_bank(dev, n_scans, n_points, seed=0):
    from eda_amd import synthetic
    rng = np.random.RandomState(seed)
    bank = A.SceneBank(dev, capacity=n_scans)
    for s in range(n_scans):
        xyz = synthetic.batch([s], n_points)[0, :, :3].astype(np.float64)
        k = rng.randint(40, 90)
        owner = np.where(rng.rand(n_points) < 0.9, rng.randint(0, k, n_points), -1)
        c = rng.uniform(-2, 2, (30, 3))
        sz = rng.uniform(0.1, 1.0, (30, 3))
        bank.add_scan(xyz, rng.rand(n_points, 3).astype(np.float32), [np.flatnonzero(owner == i) for i in range(k)],
                      detected_boxes=np.concatenate([c - sz / 2, c + sz / 2], 1),
                      detected_class_ids=rng.randint(0, 485, 30))
    return bank


def batch_args(bank, rng, B):
    slots = rng.choice(bank.n_slots, B, replace=False)
    targets = [rng.choice(bank.n_objects(int(s)), 4, replace=False) for s in slots]
    keep = rng.rand(B, 132) < 0.8
    return slots, A.draw_params(rng, B, augment_det=True), targets, keep


def time_events(fn, reps, warm=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts))


def pipe_ms(stage, bank, rng, B, N, steps):
    import bench
    import check_graph_vs_eager as C
    from eda_amd import pipeline
    from eda_amd.parallel import FlatParams
    dev = bank.device
    model = C.make(0, dev)
    flat = FlatParams(model)

    def backward(loss):
        with flat.deferred_wgrad():
            loss.backward()
        flat.collect_grads()

    def update():
        flat.clip_grad_norm_(0.1)
        with torch.no_grad():
            for gp in flat.groups.values():
                gp.add_(gp.grad, alpha=-1e-4)

    loss_fn = lambda ep, batch: bench.synthetic_loss(ep)          # noqa: E731
    base = bench.make_inputs(0, B, dev, N, 80)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            loss = loss_fn(model(base), base)
            backward(loss)
            update()
        torch.cuda.synchronize()
        feeds = [None]
        first = base
        if stage is not None:
            packs = [{k: v.to(dev) for k, v in stage.pack(*batch_args(bank, rng, B)).items()} for _ in range(4)]
            first = dict(base, **A.augment_batch(bank, *batch_args(bank, rng, B)), **packs[0])
            rest = {k: v for k, v in base.items() if k not in stage.produces}
            feeds = [dict(rest, **p) for p in packs]
        else:
            feeds = [base]
        pipe = pipeline.PipelinedTrainStep(model, first, loss_fn, backward, update, stream=side, pre_stage=stage)
        for i in range(5):
            pipe.step(next_batch=feeds[i % len(feeds)])
        torch.cuda.synchronize()
        ts = []
        for i in range(steps):
            t0 = time.perf_counter()
            pipe.step(next_batch=feeds[i % len(feeds)])
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--points", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--no-pipe", action="store_true")
    args = ap.parse_args()
    B, N = args.scenes, args.points
    rng = np.random.RandomState(0)
    out = {"scenes": B, "points": N}
    dev = torch.device("cuda", 0)
    bank = make_bank(dev, 2 * B, N)
    stage = A.AugmentStage(bank, B, detected_mode="butd", augment_det=True, seed=1)
    stage.set_inputs(*batch_args(bank, rng, B))
    out["eager_us_per_batch"] = time_events(stage, args.reps)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=side):
        stage()
    out["graph_us_per_batch"] = time_events(g.replay, args.reps)
    out["launches"] = 2
    out["bytes_read_mb"] = B * N * (24 + 12 + 2) / 1e6
    out["bytes_written_mb"] = B * N * (24 + 12 + 8) / 1e6
    # CPU form, one thread, per scene
    torch.set_num_threads(1)
    cpu_bank = A.SceneBank("cpu")
    for s in range(2):
        cpu_bank.add_scan(bank.xyz[s].cpu().numpy(), bank.color[s].cpu().numpy(),
                          [np.flatnonzero(bank.obj[s].cpu().numpy() == i) for i in range(bank.n_objects(s))],
                          detected_boxes=np.zeros((30, 6)))
    slots, params, targets, keep = [0, 1], A.draw_params(rng, 2, augment_det=True), [[0, 1], [2]], np.ones((2, 132), bool)
    A.augment_batch(cpu_bank, slots, params, targets, keep, "butd", augment_det=True)
    t0 = time.perf_counter()
    for _ in range(3):
        A.augment_batch(cpu_bank, slots, params, targets, keep, "butd", augment_det=True)
    out["cpu_ms_per_scene"] = (time.perf_counter() - t0) * 1e3 / 6
    if not args.no_pipe:
        out["pipe_ms_no_stage"] = pipe_ms(None, bank, rng, B, N, args.steps)
        stage2 = A.AugmentStage(bank, B, seed=2)
        out["pipe_ms_with_stage"] = pipe_ms(stage2, bank, rng, B, N, args.steps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
