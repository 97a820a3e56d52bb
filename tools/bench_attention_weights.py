"""Graph-replay time of the attention-map launch (csrc/mha_weights.hip) at five (Lq, Lk) sites of the model, B = 8,
against the torch form on the same device (q k^T per head, masked softmax, head mean: the only way to get these maps
without the launch), and the extra cost of GroundingSession.ground(explain=True) over ground().

usage: python tools/bench_attention_weights.py [--out FILE] [--bounds PYTEST_LOG]
  --out     write the note (markdown, stamped with bench.source_hash()) there as well as to stdout
  --bounds  a `pytest -s` log of tests/test_attention_weights_gpu.py: its ATTN_WEIGHTS_BOUND lines become the error table"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402
from eda_amd import attention  # noqa: E402

SITES = [(1024, 1024, "enc self-vis"), (80, 1024, "enc cross_lv"), (1024, 80, "enc cross_vl"),
         (256, 80, "dec cross_l"), (256, 1024, "dec cross_v")]
B, H = 8, 8


def timeit(fn, n=10):
    """Median of 5 event pairs around n calls, us per call."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / n * 1e3)
    out.sort()
    return out[2], out[-1] - out[0]


def graph_of(fn, reps):
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            for _ in range(reps):
                fn()
    return g


def kernel_rows():
    rows = []
    torch.manual_seed(0)
    for Lq, Lk, name in SITES:
        q, k, v = (torch.randn(B, L, 288, device="cuda") for L in (Lq, Lk, Lk))
        mask = torch.zeros(B, Lk, dtype=torch.bool, device="cuda")
        mask[1:, Lk - 7:] = True
        m8 = mask.view(torch.uint8)
        out = torch.empty(B, Lq, 288, device="cuda")
        lse = torch.empty(B, H, Lq, device="cuda")
        attention.dropout_state("cuda")
        attention._mha_fwd_call(q, k, v, m8, B, H, Lq, Lk, 36, 0.1, 7, out, lse)
        reps = 20
        with torch.no_grad():
            t = {}
            for key, fn in (("mean", lambda: attention._mha_weights_call(q, k, m8, lse, H, 0.0, 7, False)),
                            ("mean_drop", lambda: attention._mha_weights_call(q, k, m8, lse, H, 0.1, 7, False)),
                            ("per_head", lambda: attention._mha_weights_call(q, k, m8, lse, H, 0.0, 7, True)),
                            ("torch", lambda: attention._torch_weights(q, k, mask, H, False)),
                            ("fwd", lambda: attention._mha_fwd_call(q, k, v, m8, B, H, Lq, Lk, 36, 0.0, 7, out, lse))):
                g = graph_of(fn, reps)
                med, spread = timeit(g.replay)
                t[key] = (med / reps, spread / reps)
                del g
        flop = 2.0 * B * H * Lq * Lk * 36
        wbytes = 4.0 * B * Lq * Lk
        rows.append((name, Lq, Lk, t, flop, wbytes))
        print(f"{name:13s} {Lq:5d} x {Lk:4d}: launch {t['mean'][0]:7.2f} us (dropout {t['mean_drop'][0]:7.2f}, per head "
              f"{t['per_head'][0]:7.2f}) | torch form {t['torch'][0]:8.2f} us | forward {t['fwd'][0]:7.2f} us", flush=True)
    return rows


def explain_cost():
    import check_graph_vs_eager as C
    from eda_amd.inference import GroundingSession
    dev = torch.device("cuda", 0)
    U = 5
    model = C.make(0, dev, num_queries=256).eval()
    inputs = bench.make_inputs(3, U, dev, 50000, 24)
    scene = inputs["point_clouds"][0]
    tok = inputs["tokenized"]
    det = (inputs["det_boxes"][0], inputs["det_bbox_label_mask"][0], inputs["det_class_ids"][0])
    session = GroundingSession(model)
    with torch.no_grad():
        handle = session.ground(scene, tok, detected_boxes=det)["scene"]
        res = {}
        for _ in range(3):                                    # alternate the two forms; median of 3 x 10 calls
            for explain in (False, True):
                for _ in range(2):
                    session.ground(None, tok, detected_boxes=det, explain=explain, scene=handle)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(10):
                    session.ground(None, tok, detected_boxes=det, explain=explain, scene=handle)
                torch.cuda.synchronize()
                res.setdefault(explain, []).append((time.perf_counter() - t0) / 10 * 1e3)
    return sorted(res[False]), sorted(res[True])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--bounds")
    ap.add_argument("--no-session", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    rows = kernel_rows()
    L = ["# Attention maps: the weights launch (`csrc/mha_weights.hip`)", "",
         f"Source hash `{bench.source_hash()}` (`bench.source_hash()`: sha256 over `eda_amd/csrc`).  One MI355X, "
         "`tools/bench_attention_weights.py`: every figure is a graph replay of 20 back-to-back calls divided by 20, median "
         "of 5 event-pair measurements of 10 replays each (spread = max - min of the 5); B = 8, 8 heads x 36, fp32, a "
         "key-padding mask on the last 7 keys of 7 scenes.", "",
         "| site | Lq x Lk | launch, head mean (us) | spread | with dropout 0.1 | per head | torch form (us) | torch / launch | "
         "the forward itself (us) | GFLOP | MB written | share of fp32 MFMA peak | share of 6.3 TB/s |",
         "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for name, Lq, Lk, t, flop, wb in rows:
        us = t["mean"][0]
        L.append(f"| {name} | {Lq} x {Lk} | {us:.2f} | {t['mean'][1]:.2f} | {t['mean_drop'][0]:.2f} | {t['per_head'][0]:.2f} | "
                 f"{t['torch'][0]:.2f} | {t['torch'][0] / us:.1f} | {t['fwd'][0]:.2f} | {flop * 1e-9:.2f} | {wb * 1e-6:.1f} | "
                 f"{flop / (us * 1e-6) / 157.3e12:.2f} | {wb / (us * 1e-6) / 6.3e12:.2f} |")
    L += ["", "The torch form is `eda_amd.attention._torch_weights` on the device: fp32 q k^T per head through a (B, 8, Lq, Lk) "
          "intermediate, masked fill, softmax, head mean.  Share of peak: the QK^T FLOPs (2 B H Lq Lk 36) over 157.3 TFLOP/s "
          "and the bytes of the head-mean output over 6.3 TB/s, each over the launch time; the larger of the two says what "
          "bounds the launch."]
    if not args.no_session:
        plain, expl = explain_cost()
        L += ["", "## `GroundingSession.ground(explain=True)`", "",
              "One scene of 50 000 points (handle reused: the point backbone does not run), 5 sentences of 24 tokens, 256 "
              "queries, 6 decoder layers, eager, host clock around 10 calls with one synchronisation, 3 alternating rounds:", "",
              "| | ms per call (3 rounds, sorted) |", "|---|---|",
              "| `ground()` | " + " ".join(f"{x:.2f}" for x in plain) + " |",
              "| `ground(explain=True)` | " + " ".join(f"{x:.2f}" for x in expl) + " |", "",
              f"Median difference: {expl[1] - plain[1]:+.2f} ms (three recorded maps = three launches and two gathers; the "
              "call is host-paced, so the difference is mostly the extra Python and launch work, not kernel time)."]
    if args.bounds and os.path.exists(args.bounds):
        worst = {}
        for line in open(args.bounds):
            i = line.find("ATTN_WEIGHTS_BOUND ")
            if i < 0:
                continue
            _, what, shape, val = line[i:].split()[:4]
            worst.setdefault(what, []).append((shape, float(val)))
        L += ["", "## Measured use of the error bounds (`tests/test_attention_weights_gpu.py`, worst err / tol per case)", "",
              "| check | cases | worst use of the bound | at |", "|---|---|---|---|"]
        for what, vals in worst.items():
            shape, v = max(vals, key=lambda sv: sv[1])
            L.append(f"| {what} | {len(vals)} | {v:.3f} | {shape} |")
        L += ["", "Per shape (kernel against the fp64 restatement, bound 1e-4 |e| + 2e-6 max|e|):", "",
              "| shape | " + " | ".join(w for w in worst if w.startswith("kernel_")) + " |",
              "|---|" + "---|" * sum(1 for w in worst if w.startswith("kernel_"))]
        shapes = []
        for w, vals in worst.items():
            if w.startswith("kernel_"):
                for s, _ in vals:
                    if s not in shapes:
                        shapes.append(s)
        for s in shapes:
            L.append(f"| {s} | " + " | ".join(
                f"{dict(vals).get(s, float('nan')):.3f}" for w, vals in worst.items() if w.startswith("kernel_")) + " |")
    text = "\n".join(L) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
